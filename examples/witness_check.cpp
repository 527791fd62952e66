// The witness check from C++ (include/h2mi_flex.hpp flex::check over h2mi_prover_check): what the reference's users get from
// `MockProver::run(k, &circuit, instances).assert_satisfied()` (src/scaffold.rs:39-93), on the device at the sizes the prover runs at.
//     witness_check <k> <lookup_bits> <x> <srs_secret_hex> <none | gate>
// builds the range closure (examples/range.rs:10-34) for x, makes the keys, optionally spoils the witness (the output cell of the
// second enabled gate) and prints "check ok" or "check failed: <what>"; then proves through the same workspace.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "h2mi.hpp"
#include "h2mi_flex.hpp"

using namespace h2mi;

static Fr fr_from_hex(std::string h) {
  if (h.rfind("0x", 0) == 0) h = h.substr(2);
  h = std::string(64 > h.size() ? 64 - h.size() : 0, '0') + h;
  if (h.size() > 64) h = h.substr(h.size() - 64);
  Fr raw;
  for (int i = 0; i < 4; i++) raw.l[i] = std::stoull(h.substr(64 - 16 * (i + 1), 16), nullptr, 16);
  return fr::mul(raw, fr::R2);
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: witness_check <k> <lookup_bits> <x> <srs_secret_hex> <none | gate>\n");
    return 1;
  }
  const uint32_t k = (uint32_t)std::atoi(argv[1]), lookup_bits = (uint32_t)std::atoi(argv[2]);
  const uint64_t x = std::stoull(argv[3], nullptr, 0);
  const Fr s = fr_from_hex(argv[4]);
  const std::string spoil = argv[5];
  try {
    init();
    auto params = poly::kzg::ParamsKZG::setup(k, s);
    const flex::FlexGateCS cs(true);
    auto pk = flex::keygen(params, cs, flex::range_closure(cs, 0, lookup_bits, 1));
    flex::Assignment asg = flex::range_closure(cs, x, lookup_bits, 1);
    flex::mock(asg, k);
    if (spoil == "gate") {
      auto it = asg.fixed[cs.col_qs[0]].begin();
      ++it;
      Fr& cell = asg.advice[0][it->first + 3];
      cell = fr::add(cell, fr::ONE);
    } else if (spoil != "none") {
      std::fprintf(stderr, "witness_check: unknown choice %s\n", spoil.c_str());
      return 1;
    }
    flex::FlexWorkspace ws(params, *pk);
    int rc = 0;
    try {
      flex::check(params, *pk, asg, 1, &ws);
      std::printf("check ok\n");
    } catch (const Error& e) {
      if (e.code != H2MI_EUNSAT) throw;
      std::printf("check failed: %s\n", e.what());
      rc = 3;
    }
    // the workspace proves on: the check abandons nothing and leaves nothing behind
    auto transcript = transcript::Blake2bWrite::init();
    flex::create_proof(params, *pk, flex::range_closure(cs, x, lookup_bits, 1), 1, transcript, &ws);
    std::printf("proof_bytes %zu\n", transcript.finalize().size());
    h2mi_shutdown();
    return rc;
  } catch (const Error& e) {
    std::fprintf(stderr, "witness_check: %s\n", e.what());
    return 2;
  }
}
