// The key-file parser (halo2-scaffold_amd/csrc/h2mi_keyfile.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its
// own: g++ -std=c++17 -fsanitize=address,undefined sanitize_keyfile.cpp, no library, no GPU.  tests/test_key_file_host.py writes its
// blobs — the well-formed ones and every tampered one — into files and names them on the command line; each is read into a heap block
// of exactly its length (a read one byte past the end is a report), parsed there and once more from an odd address, and its verdict
// printed as "<file name> <return code>".  The rule lines in front print the header's layout and int64 rules at the values the test
// asks for, so that the same numbers are compared with the Python reference.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../halo2-scaffold_amd/csrc/h2mi_keyfile.hpp"

using namespace h2mi::keyfile;

static int parse_file(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(3);
  }
  std::vector<uint8_t> bytes;
  uint8_t chunk[4096];
  for (size_t n; (n = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + n);
  std::fclose(f);
  uint8_t* exact = (uint8_t*)std::malloc(bytes.size() ? bytes.size() : 1);
  if (!bytes.empty()) std::memcpy(exact, bytes.data(), bytes.size());
  Blob a;
  const int rc = parse(exact, bytes.size(), a);
  std::free(exact);
  uint8_t* odd = (uint8_t*)std::malloc(bytes.size() + 1);
  if (!bytes.empty()) std::memcpy(odd + 1, bytes.data(), bytes.size());
  Blob b;
  const int rc_odd = parse(odd + 1, bytes.size(), b);
  std::free(odd);
  if (rc != rc_odd) {
    std::fprintf(stderr, "%s: %d from an aligned copy, %d from an odd address\n", path, rc, rc_odd);
    std::exit(4);
  }
  if (rc == H2MI_OK) {  // a round trip through the header's own writer for the parts it can rebuild without the cells
    Writer w;
    w.header(a.logup ? FLAG_LOGUP : 0);
    w.constraint_system(a.cs, a.has_lookups);
    if (w.b.size() > bytes.size() || std::memcmp(w.b.data() + 32, bytes.data() + 32, w.b.size() - 32)) {
      std::fprintf(stderr, "%s: the writer does not reproduce the constraint system it parsed\n", path);
      std::exit(5);
    }
  }
  return rc;
}

int main(int argc, char** argv) {
  // layout <count> <last> <width> ... and word <64 hex digits, little-endian bytes> ... come first, files behind "--"
  int i = 1;
  for (; i < argc && std::string(argv[i]) != "--"; i++) {
    const std::string a = argv[i];
    if (a == "layout" && i + 3 < argc) {
      const uint64_t count = std::strtoull(argv[i + 1], nullptr, 10), last = std::strtoull(argv[i + 2], nullptr, 10), width = std::strtoull(argv[i + 3], nullptr, 10);
      std::printf("layout %llu %llu %llu %u\n", (unsigned long long)count, (unsigned long long)last, (unsigned long long)width, layout_of(count, last, width));
      i += 3;
    } else if (a == "word" && i + 1 < argc) {
      const std::string hex = argv[i + 1];
      uint8_t w[32] = {0};
      for (size_t b = 0; b < 32 && 2 * b + 1 < hex.size(); b++) w[b] = (uint8_t)std::strtoul(hex.substr(2 * b, 2).c_str(), nullptr, 16);
      std::printf("word %s %d\n", hex.c_str(), classify(w));
      i += 1;
    }
  }
  for (i++; i < argc; i++) {
    const std::string path = argv[i];
    std::printf("%s %d\n", path.substr(path.find_last_of('/') + 1).c_str(), parse_file(argv[i]));
  }
  std::printf("sanitize_keyfile: done\n");
  return 0;
}
