// fr::batch_invert_skip_zero (include/h2mi.hpp) on the canonical integers given as 64-digit hex words in argv: prints one line per
// element, its inverse as a canonical integer (zero for zero), then the line "plain" followed by what fr::batch_invert makes of the same
// input — the function the zero-skipping one stands beside and leaves alone.
#include <cstdio>
#include <string>
#include <vector>

#include "h2mi.hpp"

using h2mi::Fr;
namespace fr = h2mi::fr;

static void print(const std::vector<Fr>& v) {
  const Fr one = {{1, 0, 0, 0}};
  for (const Fr& m : v) {
    const Fr c = fr::mul(m, one);  // out of the Montgomery form
    std::printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)c.l[3], (unsigned long long)c.l[2], (unsigned long long)c.l[1],
                (unsigned long long)c.l[0]);
  }
}

int main(int argc, char** argv) {
  std::vector<Fr> v;
  for (int i = 1; i < argc; i++) {
    const std::string hex = argv[i];
    if (hex.size() != 64) return 2;
    Fr c;
    for (int j = 0; j < 4; j++) c.l[3 - j] = std::stoull(hex.substr(16 * j, 16), nullptr, 16);
    v.push_back(fr::mul(c, fr::R2));
  }
  print(fr::batch_invert_skip_zero(v));
  std::printf("plain\n");
  print(fr::batch_invert(v));
  return 0;
}
