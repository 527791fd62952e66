"""The C++ host (include/h2mi_plonk.hpp) with plonk::MultiOpen::GWC: a small program (tests/host/gwc_plonk.cpp) built against the header
and the in-tree library gives, for the same seed, the bytes the Python host gives — and its SHPLONK proof between two GWC proofs on one
workspace is the Python host's SHPLONK proof."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_gives_the_python_hosts_bytes(gpu, tmp_path):
    from halo2_scaffold_amd import circuits, keygen, prover

    libdir = os.path.join(ROOT, "halo2-scaffold_amd")
    exe = str(tmp_path / "gwc_plonk")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "gwc_plonk.cpp"),
                           "-L" + libdir, "-lh2mi", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    k, secret, xw, seed = 5, 0x5EC2E7, 0xC0FFEE, 11
    r = subprocess.run([exe, str(k), "%x" % secret, "%x" % xw, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    params = gpu.ParamsKZG.setup(k, secret)
    circuit = circuits.StandardPlonk(None)
    pk = keygen.keygen_pk(params, keygen.keygen_vk(params, circuit), circuit)
    shplonk = prover.create_proof(params, pk, circuits.StandardPlonk(xw), seed)
    gwc = prover.create_proof(params, pk, circuits.StandardPlonk(xw), seed, multiopen="gwc")
    assert out["gwc"] == out["gwc_again"] == gwc.hex() and out["shplonk"] == shplonk.hex()
    assert len(gwc) == len(shplonk) - 64 + 32 * 3 and gwc[:-96] == shplonk[:-64]  # three permutation sets: x, omega x and x_last, P = 3
    pk.release()
    params.release()
