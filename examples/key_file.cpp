// "In production the proving key is generated only once" (the reference on gen_key): the StandardPlonk key of
// examples/standard_plonk.cpp made by keygen, written to a file (plonk::ProvingKey::write: h2mi_prover_pk_export), read back into a
// FRESH key after the first one is released (plonk::ProvingKey::read: h2mi_prover_pk_import — no synthesis, the commitments recomputed
// and compared with the stored ones), and a proof made against each.  The two proofs are the same bytes; so is the proof the Python
// host makes for the same arguments (tests/test_gpu_key_file.py runs this program and compares).
//
// Usage: key_file <path> [k [srs_secret_hex [witness_hex [seed]]]]
#include <cstdio>
#include <fstream>
#include <string>

#include "../include/h2mi_plonk.hpp"

using namespace h2mi;

static Fr fr_from_hex(std::string h) {  // canonical integer -> Fr, as examples/standard_plonk.cpp reads its arguments
  if (h.rfind("0x", 0) == 0) h = h.substr(2);
  while (h.size() < 64) h = "0" + h;
  if (h.size() > 64) h = h.substr(h.size() - 64);
  Fr raw;
  for (int i = 0; i < 4; i++) raw.l[i] = std::stoull(h.substr(64 - 16 * (i + 1), 16), nullptr, 16);
  return fr::mul(raw, fr::R2);
}
static std::string hex(const std::vector<uint8_t>& b) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint8_t c : b) {
    s.push_back(d[c >> 4]);
    s.push_back(d[c & 15]);
  }
  return s;
}
static std::vector<uint8_t> prove(const poly::kzg::ParamsKZG& params, const plonk::ProvingKey& pk, const Fr& x, uint64_t seed) {
  auto transcript = transcript::Blake2bWrite::init();
  plonk::create_proof(params, pk, plonk::StandardPlonk(x), seed, transcript);
  return transcript.finalize();
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: key_file <path> [k [srs_secret_hex [witness_hex [seed]]]]\n");
    return 1;
  }
  const std::string path = argv[1];
  const uint32_t k = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 5;
  const Fr s = fr_from_hex(argc > 3 ? argv[3] : "5ec2e7");
  const Fr x = fr_from_hex(argc > 4 ? argv[4] : "c0ffee");
  const uint64_t seed = argc > 5 ? std::stoull(argv[5]) : 11;
  try {
    init();
    auto params = poly::kzg::ParamsKZG::setup(k, s);
    std::vector<uint8_t> made;
    {  // keygen, prove, write; the key is released at the end of the block
      plonk::StandardPlonk circuit;
      auto pk = plonk::keygen_pk(params, plonk::keygen_vk(params, circuit), circuit);
      made = prove(params, *pk, x, seed);
      std::ofstream out(path, std::ios::binary);
      pk->write(out);
      if (!out) throw Error(H2MI_EINVAL, "cannot write " + path);
    }
    std::ifstream in(path, std::ios::binary);
    if (!in) throw Error(H2MI_EINVAL, "cannot read " + path);
    auto pk = plonk::ProvingKey::read(params, in);  // a fresh key: no keygen, no synthesis
    const std::vector<uint8_t> loaded = prove(params, *pk, x, seed);
    std::printf("vk %s\n", hex(pk->get_vk().to_bytes()).c_str());
    std::printf("proof %s\n", hex(loaded).c_str());
    std::printf("same_as_the_generated_key %d\n", made == loaded ? 1 : 0);
    pk.reset();
    h2mi_shutdown();
    return made == loaded ? 0 : 3;
  } catch (const Error& e) {
    std::fprintf(stderr, "key_file: %s\n", e.what());
    return 2;
  }
}
