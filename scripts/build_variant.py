"""Build a compile-time variant of libsrbd_mpc.so into OUT, on the CPU host.

    python scripts/build_variant.py OUT [--no-regn] [--reg20=FLAG ...] [-DFLAG | compiler flag ...]

A variant is the product build perturbed: biped_pympc_amd/build.py build_core compiles every unit of
HIP_UNITS with the product's per-unit flags (N = 20 in its own unit under the register-pressure
trackers) and adds the given flags on top, to every unit. That is the shipped configuration, so with
no flags the device code is the product's; the build id is the product's only for identical sources
and flags.
--reg20=FLAG adds FLAG to the N = 20 unit only (e.g. --reg20=-include --reg20=scripts/phase_prof.hpp:
the phase stamps of the N = 20 kernels, whose accumulators then live in that unit alone).
--no-regn compiles scripts/regn_stub.hip in place of the srbd_regN.hip unit (half a minute instead of
four): the horizons other than 10 and 20 then run the LDS-resident kernels (N = 10 / 20 experiments only).
The other variant tools import this module. Diagnostic tool: the product library is only ever built by biped_pympc_amd/build.py.
"""
import contextlib
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from biped_pympc_amd.build import CSRC, INCLUDE, build_core  # noqa: E402

REGN_STUB = os.path.join(ROOT, "scripts", "regn_stub.hip")
PHASE_PROF = ["-include", os.path.join(ROOT, "scripts", "phase_prof.hpp")]  # for one unit only (unit_flags)


def needs_regn(*horizons) -> bool:
    """Whether a run at these horizons needs the real srbd_regN.hip unit (any horizon but 10 and 20)."""
    return any(int(n) not in (10, 20) for n in horizons)


def reg_unit(horizon) -> str:
    """The unit that holds the register kernels of a horizon."""
    return {10: "srbd_mpc.hip", 20: "srbd_reg20.hip"}.get(int(horizon), "srbd_regN.hip")


def build_variant(out: str, flags=(), regn: bool = True, reg20_flags=(), unit_flags: dict | None = None,
                  csrc: str | None = None) -> dict:
    """Returns build_core's {unit: command line} of what it compiled."""
    uf = {u: list(f) for u, f in (unit_flags or {}).items()}
    if reg20_flags:
        uf["srbd_reg20.hip"] = uf.get("srbd_reg20.hip", []) + list(reg20_flags)
    return build_core(out, csrc=csrc, flags=list(flags), unit_flags=uf,
                      replace=None if regn else {"srbd_regN.hip": REGN_STUB})


@contextlib.contextmanager
def patched_csrc(patch, header: str = "pdipm_srbd_reg.hpp"):
    """A temporary copy of the sources (biped_pympc_amd/csrc + include, the layout srbd_mpc.hip's
    relative include needs) with `header` rewritten by patch(text) -> text; yields the copy's csrc for
    build_variant(csrc=). The product sources are never modified."""
    with tempfile.TemporaryDirectory() as td:
        d = os.path.join(td, "biped_pympc_amd", "csrc")
        shutil.copytree(CSRC, d)
        shutil.copytree(INCLUDE, os.path.join(td, "include"))
        p = os.path.join(d, header)
        src = open(p).read()
        new = patch(src)
        assert new != src, f"{header}: the patch changed nothing"
        open(p, "w").write(new)
        yield d


if __name__ == "__main__":
    args = sys.argv[2:]
    r20 = [a[len("--reg20="):] for a in args if a.startswith("--reg20=")]
    rest = [a for a in args if a != "--no-regn" and not a.startswith("--reg20=")]
    build_variant(sys.argv[1], rest, regn="--no-regn" not in args, reg20_flags=r20)
    print(sys.argv[1])
