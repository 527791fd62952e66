// AddressSanitizer / UndefinedBehaviorSanitizer run of the raw-limb point operations (f29t_point_raw over csrc/g1_29.cuh) on the
// cases of tests/g1_29_edge_cases.py: operands at the bounds of the coordinate invariants are where a limb-wise subtraction would
// wrap or a shift would overflow.  A program of its own (sanitizers run on the CPU build, never inside Python):
//     g1_29_edges_main <cases file> <results file>
// cases file: per op { uint32 op, uint32 n, a[n][36], b[n][36] } (uint32 words) until the end of the file; the results file gets
// out[n][36] per op in the same order.  Built and run by tests/test_g1_29_edges_host.py, which compares the results with the
// unsanitized build's.  Test infrastructure, not product.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "f29_host.cpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* res = fopen(argv[2], "wb");
  if (!in || !res) return 2;
  uint32_t head[2];
  size_t total = 0;
  while (fread(head, 4, 2, in) == 2) {
    const size_t n = head[1];
    std::vector<uint32_t> a(36 * n), b(36 * n), out(36 * n);
    if (fread(a.data(), 4, 36 * n, in) != 36 * n || fread(b.data(), 4, 36 * n, in) != 36 * n) return 3;
    f29t_point_raw((int)head[0], a.data(), b.data(), out.data(), n);
    if (fwrite(out.data(), 4, 36 * n, res) != 36 * n) return 4;
    total += n;
  }
  fclose(in);
  if (fclose(res) != 0) return 4;
  printf("%zu elements\n", total);
  return 0;
}
