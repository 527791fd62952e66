// Yardstick for h2mi_fr_sort_unique_dev (csrc/h2mi_lookup.hip): rocprim::merge_sort over the same keys with the same 256-bit
// comparison.  A standalone program: the product does not link rocPRIM; this tool loads libh2mi.so at run time and includes
// rocPRIM's headers from the ROCm include tree.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -o tools/sort_yardstick tools/sort_yardstick.hip -ldl
//   run:   tools/sort_yardstick halo2-scaffold_amd/libh2mi.so [repeats = 11]
// Per size (2^16, 2^20) and key class (uniform; the 16-bit counting table padded with zeros): `repeats` interleaved pairs of
// calls after two warm-up pairs, each timed on the host clock between device synchronisations; medians with min .. max.
// The library call is timed whole: Montgomery -> canonical, the sort, distinct values and multiplicities, its two read-backs.
// rocPRIM sorts keys that are canonical already and does nothing else.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <rocprim/device/device_merge_sort.hpp>
#include <vector>

struct Key {
  uint32_t v[8];
};
struct KeyLess {
  __host__ __device__ bool operator()(const Key& a, const Key& b) const {
    for (int i = 7; i >= 0; i--)
      if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
    return false;
  }
};
#define CK(x)                                                            \
  do {                                                                   \
    hipError_t e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                              \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));           \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static const uint64_t MODULUS[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t MONT_ONE[4] = {0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full};
static void add_mod(uint64_t a[4], const uint64_t b[4]) {  // a = a + b mod r, both below r
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (unsigned __int128)a[i] + b[i];
    a[i] = (uint64_t)c;
    c >>= 64;
  }
  bool ge = true;
  for (int i = 3; i >= 0; i--)
    if (a[i] != MODULUS[i]) {
      ge = a[i] > MODULUS[i];
      break;
    }
  if (!ge) return;
  unsigned __int128 bw = 0;
  for (int i = 0; i < 4; i++) {
    const unsigned __int128 d = (unsigned __int128)a[i] - MODULUS[i] - (uint64_t)bw;
    a[i] = (uint64_t)d;
    bw = (d >> 64) & 1;
  }
}

typedef int (*init_fn)(int);
typedef int (*sort_fn)(const void*, uint32_t, void*, void*, void*, uint32_t*, void*);

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <libh2mi.so> [repeats]\n", argv[0]);
    return 2;
  }
  const int reps = argc > 2 ? atoi(argv[2]) : 11;
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
  if (!lib) {
    fprintf(stderr, "%s\n", dlerror());
    return 2;
  }
  init_fn init = (init_fn)dlsym(lib, "h2mi_init");
  sort_fn sort_unique = (sort_fn)dlsym(lib, "h2mi_fr_sort_unique_dev");
  if (!init || !sort_unique || init(0)) {
    fprintf(stderr, "libh2mi.so: h2mi_init / h2mi_fr_sort_unique_dev\n");
    return 2;
  }
  std::mt19937_64 rng(12345);
  for (int log_n : {16, 20}) {
    const size_t n = (size_t)1 << log_n;
    for (int cls = 0; cls < 2; cls++) {
      // canonical keys for rocPRIM, the same values in Montgomery form for the library
      std::vector<uint64_t> canon(4 * n, 0), mont(4 * n, 0);
      if (cls == 0) {
        for (size_t i = 0; i < n; i++) {  // any words below r are the Montgomery form of a uniform element; rocPRIM sorts equally uniform keys
          for (int w = 0; w < 4; w++) mont[4 * i + w] = canon[4 * i + w] = rng();
          mont[4 * i + 3] = canon[4 * i + 3] &= 0x1fffffffffffffffull;
        }
      } else {
        uint64_t acc[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < std::min<size_t>(n, 65536); i++) {
          canon[4 * i] = i;
          for (int w = 0; w < 4; w++) mont[4 * i + w] = acc[w];
          add_mod(acc, MONT_ONE);
        }
      }
      void *d_canon, *d_mont, *d_out, *d_o1, *d_o2, *d_o3, *d_tmp = nullptr;
      CK(hipMalloc(&d_canon, n * 32));
      CK(hipMalloc(&d_mont, n * 32));
      CK(hipMalloc(&d_out, n * 32));
      CK(hipMalloc(&d_o1, n * 32));
      CK(hipMalloc(&d_o2, n * 32));
      CK(hipMalloc(&d_o3, n * 4));
      CK(hipMemcpy(d_canon, canon.data(), n * 32, hipMemcpyHostToDevice));
      CK(hipMemcpy(d_mont, mont.data(), n * 32, hipMemcpyHostToDevice));
      size_t tmp_bytes = 0;
      CK(rocprim::merge_sort(nullptr, tmp_bytes, (Key*)d_canon, (Key*)d_out, n, KeyLess(), (hipStream_t)0));
      CK(hipMalloc(&d_tmp, tmp_bytes));
      std::vector<double> t_roc, t_lib;
      uint32_t n_unique = 0;
      for (int r = 0; r < reps + 2; r++) {
        CK(hipDeviceSynchronize());
        auto t0 = std::chrono::steady_clock::now();
        CK(rocprim::merge_sort(d_tmp, tmp_bytes, (Key*)d_canon, (Key*)d_out, n, KeyLess(), (hipStream_t)0));
        CK(hipDeviceSynchronize());
        auto t1 = std::chrono::steady_clock::now();
        if (sort_unique(d_mont, (uint32_t)n, d_o1, d_o2, d_o3, &n_unique, nullptr)) {
          fprintf(stderr, "h2mi_fr_sort_unique_dev failed\n");
          return 1;
        }
        CK(hipDeviceSynchronize());
        auto t2 = std::chrono::steady_clock::now();
        if (r >= 2) {
          t_roc.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
          t_lib.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
        }
      }
      if (cls == 1) {  // the two must agree on the distinct values: the first key of every run of rocPRIM's output
        std::vector<uint64_t> a(4 * n), b(4 * (size_t)n_unique);
        CK(hipMemcpy(a.data(), d_out, n * 32, hipMemcpyDeviceToHost));
        CK(hipMemcpy(b.data(), d_o1, (size_t)n_unique * 32, hipMemcpyDeviceToHost));
        size_t u = 0;
        bool same = true;
        for (size_t i = 0; i < n; i++) {
          if (i && std::equal(&a[4 * i], &a[4 * i + 4], &a[4 * (i - 1)])) continue;
          same = same && u < n_unique && std::equal(&a[4 * i], &a[4 * i + 4], &b[4 * u]);
          u++;
        }
        if (!same || u != n_unique) {
          fprintf(stderr, "distinct values differ\n");
          return 1;
        }
      }
      std::sort(t_roc.begin(), t_roc.end());
      std::sort(t_lib.begin(), t_lib.end());
      printf("2^%d %-8s n_unique %8u  rocprim::merge_sort %9.1f us (%.1f .. %.1f)   h2mi_fr_sort_unique_dev %9.1f us (%.1f .. %.1f)   ratio %.2f\n", log_n,
             cls ? "counting" : "uniform", n_unique, t_roc[reps / 2], t_roc.front(), t_roc.back(), t_lib[reps / 2], t_lib.front(), t_lib.back(),
             t_lib[reps / 2] / t_roc[reps / 2]);
      for (void* p : {d_canon, d_mont, d_out, d_o1, d_o2, d_o3, d_tmp}) CK(hipFree(p));
    }
  }
  return 0;
}
