"""Static audit of the DPP wait states in the test-only primitive harness (CPU only).

tests/csrc/prim_harness.hip wraps each building block of the DPP row kernels in a trivial kernel. The
broadcast-FMA asm blocks carry no trailing wait states (csrc/dpp_rows.hpp), so a harness kernel could
itself place a DPP read within 2 wait states of a VALU write next to a block -- and then test a value
the product never computes. The same checker that audits the product units
(tests/test_isa_hazards.py, scripts/dpp_hazard_check.py) runs on the harness ISA, compiled with the
flags of the harness build. Where hipcc exists the audit must run: it fails rather than skips.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_harness_has_no_dpp_read_within_two_states_of_a_write(tmp_path):
    from biped_pympc_amd.build import HIPCC, prim_harness_compile_cmd
    from dpp_hazard_check import check
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    out = tmp_path / "prim_harness.s"
    r = subprocess.run(prim_harness_compile_cmd(["--cuda-device-only", "-S", "-o", str(out)]),
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    # the audit saw the kernels it is about: the fused broadcast-FMAs and the DPP moves are there
    assert "v_fmac_f64_dpp" in text and "row_newbcast" in text and "row_shl:6" in text
    assert check(str(out)) == 0


def test_harness_is_not_a_product_source():
    """The harness lives outside csrc/: no source of the product library, whose build id is hashed over
    them, sits in its directory."""
    from biped_pympc_amd import build as b
    assert all(os.path.dirname(s) != os.path.dirname(b.PRIM_HARNESS_SRC) for s in b.core_sources())
