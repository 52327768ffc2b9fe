"""The one build recipe (biped_pympc_amd/build.py build_core) as the variant tools use it: a variant
built by scripts/build_variant.py with no extra flags and without the srbd_regN.hip unit (the
quickest one, ~35 s of hipcc) links every unit of HIP_UNITS, loads, exports the whole C-ABI and
carries its own build id; on the GPU it computes the product's bits at the horizons it serves (same
sources, same flags: what every `base=` leg of an A/B run assumes).

    python -m tests.test_variant_build OUTDIR    the GPU test's child: runs _solves into OUTDIR with
                                                 whatever library SRBD_LIB names
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from biped_pympc_amd import build
from tests.test_native_abi import _declared_functions, _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def variant(tmp_path_factory):
    """(path, {unit: command line}) of a stub variant with no extra flags."""
    from build_variant import build_variant
    out = str(tmp_path_factory.mktemp("variant") / "libsrbd_mpc_variant.so")
    return out, build_variant(out, regn=False)


def test_variant_links_every_unit_and_exports_the_abi(variant):
    path, _ = variant
    undef = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True, check=True).stdout
    assert [l for l in undef.splitlines() if "srbd" in l] == []
    missing = (_declared_functions() - {"evaluate"}) - _exports(path)
    assert not missing, missing
    assert ctypes.CDLL(path).srbd_abi_version() == 1


def test_variant_carries_its_own_build_id(variant):
    """The stub replaced a unit, so the id is not the product's; file and srbd_build_id() agree."""
    path, _ = variant
    L = ctypes.CDLL(path)
    L.srbd_build_id.restype = ctypes.c_char_p
    assert L.srbd_build_id().decode() == build.embedded_id(path) != build.source_hash()


def test_variant_compiles_exactly_the_product_units(variant):
    """Every unit of HIP_UNITS, each with the product's command line up to the output, the stub's
    path and the variant's id."""
    _, cmds = variant
    assert set(cmds) == set(build.HIP_UNITS)
    for unit, cmd in cmds.items():
        head = [build.HIPCC, f"--offload-arch={build.ARCH}", *build._COMMON_FLAGS, *build.HIP_UNITS[unit], "-fPIC", "-c"]
        assert cmd[:len(head)] == head, cmd
        src = os.path.join(ROOT, "scripts", "regn_stub.hip") if unit == "srbd_regN.hip" else os.path.join(build.CSRC, unit)
        assert cmd[-1] == src
        assert ("-DSRBD_BUILD_ID" in " ".join(cmd)) == (unit == "srbd_mpc.hip")


def test_up_to_date_product_build_compiles_nothing(capsys):
    build.build()
    capsys.readouterr()
    build.build(verbose=True)
    assert capsys.readouterr().out == ""


def test_source_hash_covers_sources_units_and_common_flags_only():
    """The product's id depends on the sources, HIP_UNITS and _COMMON_FLAGS and on nothing else in
    build.py, so code added there leaves the id -- and the shipped library -- as it is."""
    parts = [build.ARCH, repr(sorted(build.HIP_UNITS.items())), repr(build._COMMON_FLAGS)]
    for s in build.core_sources():
        parts += [os.path.basename(s), open(s, "rb").read()]
    assert build.source_hash() == build._digest(parts)
    assert build.core_sources()[-1] == os.path.join(build.INCLUDE, "srbd_mpc.h")


def _solves(outdir):
    """mpc_solve at N = 10 and 20 (B = 3, K = 3) and mpc_backward at N = 10 on its iterate, saved as
    .npy: the smallest calls that enter all four units (N = 10 register kernels in the main unit, the
    N = 20 unit, the backward unit; a stub variant has no other register horizon)."""
    import torch
    from biped_pympc_amd import solver
    from biped_pympc_amd.utils.synthetic import make_workload
    for N in (10, 20):
        ins = [torch.from_numpy(a).cuda() for a in make_workload(3, N, seed=31 + N).inputs]
        out = solver.mpc_solve(ins, N, 3)
        names = [f"solve{N}_{k}" for k in range(len(out))]
        if N == 10:
            g = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 24 * N))).cuda()
            grads = solver.mpc_backward(ins, out[:4], g, N)
            out, names = list(out) + list(grads), names + [f"backward{N}_{k}" for k in range(len(grads))]
        torch.cuda.synchronize()
        for n, t in zip(names, out):
            np.save(os.path.join(outdir, n + ".npy"), t.cpu().numpy())


@pytest.mark.gpu
def test_variant_computes_the_products_bits(variant, tmp_path):
    """The variant runs in a fresh child process (_native binds one library per process), the
    product in this one."""
    from biped_pympc_amd import _native
    assert _native.lib_path() == os.path.join(build.LIB_DIR, "libsrbd_mpc.so")
    dirs = {n: tmp_path / n for n in ("variant", "product")}
    for d in dirs.values():
        d.mkdir()
    r = subprocess.run([sys.executable, "-m", "tests.test_variant_build", str(dirs["variant"])], cwd=ROOT,
                       env={**os.environ, "SRBD_LIB": variant[0]}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _solves(str(dirs["product"]))
    files = sorted(os.listdir(dirs["product"]))
    assert len(files) == 2 * 6 + 17 and files == sorted(os.listdir(dirs["variant"]))
    for f in files:
        a, b = np.load(dirs["product"] / f), np.load(dirs["variant"] / f)
        assert a.size and np.array_equal(a, b), f  # (a NaN equals nothing: it fails too)


if __name__ == "__main__":
    _solves(sys.argv[1])
