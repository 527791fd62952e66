// C++ host over include/h2mi_plonk.hpp with the GWC multi-opening (plonk::MultiOpen::GWC), for tests/test_gpu_gwc_cpp.py: the
// reference's StandardPlonk circuit, one GWC proof, one SHPLONK proof and the GWC proof again through ONE workspace.
// Usage: gwc_plonk k srs_secret_hex witness_hex seed   ->   lines "gwc <hex>", "shplonk <hex>", "gwc_again <hex>"
#include <cstdio>
#include <string>

#include "h2mi_plonk.hpp"

using namespace h2mi;

static Fr fr_from_hex(std::string h) {  // canonical integer -> Montgomery form
  while (h.size() < 64) h = "0" + h;
  Fr raw;
  for (int i = 0; i < 4; i++) raw.l[i] = std::stoull(h.substr(64 - 16 * (i + 1), 16), nullptr, 16);
  return fr::mul(raw, fr::R2);
}

int main(int argc, char** argv) {
  if (argc != 5) return 1;
  try {
    init();
    auto params = poly::kzg::ParamsKZG::setup((uint32_t)std::atoi(argv[1]), fr_from_hex(argv[2]));
    plonk::StandardPlonk keygen_circuit;
    plonk::VerifyingKey vk = plonk::keygen_vk(params, keygen_circuit);
    auto pk = plonk::keygen_pk(params, vk, keygen_circuit);
    plonk::StandardPlonk circuit(fr_from_hex(argv[3]));
    const uint64_t seed = std::stoull(argv[4]);
    plonk::ProverWorkspace ws(params, *pk);
    const std::pair<const char*, plonk::MultiOpen> runs[] = {{"gwc", plonk::MultiOpen::GWC}, {"shplonk", plonk::MultiOpen::SHPLONK}, {"gwc_again", plonk::MultiOpen::GWC}};
    for (const auto& run : runs) {
      auto transcript = transcript::Blake2bWrite::init();
      plonk::create_proof(params, *pk, circuit, seed, transcript, &ws, run.second);
      std::printf("%s ", run.first);
      for (uint8_t c : transcript.finalize()) std::printf("%02x", c);
      std::printf("\n");
    }
    h2mi_shutdown();
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "gwc_plonk: %s\n", e.what());
    return 2;
  }
}
