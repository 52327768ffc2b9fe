"""Build the native libraries in-tree (hipcc for gfx950 + gcc for the thin CusADi-ABI shims).

Outputs (biped_pympc_amd/lib/):
  libsrbd_mpc.so                                  HIP kernels + extended C-ABI (include/srbd_mpc.h)
  libqp_former.so                                 CusADi `evaluate` for 'qp_former' (N = 10)
  libsparse_pdipm_multiple_iterations.so          CusADi `evaluate` for the deployed solver (N=10, 5 it)
  libqp_former_N<N>.so, libsparse_pdipm_multiple_iterations_N<N>_K<K>.so   other configurations
Replaces the reference's CasADi -> CUDA codegen + CMake pipeline (run_codegen.py:9-44), which
takes ~3 h for 5 unrolled Newton iterations (README.md:80-84); this builds in seconds.
"""
from __future__ import annotations

import contextlib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB_DIR = os.path.join(PKG, "lib")
INCLUDE = os.path.join(ROOT, "include")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("SRBD_OFFLOAD_ARCH", "gfx950")

# (function name, N, K) of the thin CusADi-ABI libraries to build
DROPIN_CONFIGS = [
    ("qp_former", 10, None),
    ("sparse_pdipm_multiple_iterations", 10, 5),
    ("qp_former", 20, None),
    ("sparse_pdipm_multiple_iterations", 10, 10),
    ("sparse_pdipm_multiple_iterations", 20, 10),
]


def dropin_lib_name(fn: str, N: int, K: int | None) -> str:
    if fn == "qp_former":
        return "libqp_former.so" if N == 10 else f"libqp_former_N{N}.so"
    if N == 10 and K == 5:
        return "libsparse_pdipm_multiple_iterations.so"
    return f"libsparse_pdipm_multiple_iterations_N{N}_K{K}.so"


_ID_RE = re.compile(rb"srbd-(build|shim)-id:([0-9a-f]{16})")


def embedded_id(path: str) -> str | None:
    """The build id a library carries ("srbd-build-id:<16 hex>" in libsrbd_mpc.so's read-only data,
    "srbd-shim-id:<16 hex>" in a drop-in), read from the file without loading it; None if absent."""
    try:
        with open(path, "rb") as fh:
            m = _ID_RE.search(fh.read())
    except OSError:
        return None
    return m.group(2).decode() if m else None


def _digest(parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else str(p).encode())
        h.update(b"\0")
    return h.hexdigest()[:16]


def core_sources(csrc: str | None = None) -> list[str]:
    """Every file libsrbd_mpc.so is compiled from: the HIP units, their headers, the C-ABI header
    (which srbd_mpc.hip includes as ../../include/srbd_mpc.h, so it is found relative to `csrc`)."""
    csrc = os.path.abspath(csrc or CSRC)
    srcs = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp"))]
    return srcs + [os.path.join(os.path.dirname(os.path.dirname(csrc)), "include", "srbd_mpc.h")]


def source_hash(sources: list[str] | None = None) -> str:
    """Build id of libsrbd_mpc.so: sha256 over the sources' names and bytes and the compile flags,
    truncated to 16 hex digits. Embedded in the library (srbd_build_id()); build() rebuilds when the
    library's id differs from this, whatever the files' mtimes say."""
    parts = [ARCH, repr(sorted(HIP_UNITS.items())), repr(_COMMON_FLAGS)]
    for s in core_sources() if sources is None else sources:
        parts += [os.path.basename(s), open(s, "rb").read()]
    return _digest(parts)


def _unit_hash(unit: str, cmd: list[str], sources: list[str]) -> str:
    """What one object file depends on: its flags (for the main unit they carry the library's build
    id, which it embeds), its source and every header (csrc/*.hpp; include/srbd_mpc.h for the main and
    the backward unit, the two that include it)."""
    parts = [unit, repr(cmd[1:cmd.index("-o")])]
    for s in [cmd[-1]] + [h for h in sources if not h.endswith(".hip")]:
        if s.endswith(".h") and unit not in ("srbd_mpc.hip", "srbd_backward.hip"):
            continue
        parts += [os.path.basename(s), open(s, "rb").read()]
    return _digest(parts)


def _shim_hash(fn: str, N: int, K: int | None, core_id: str) -> str:
    shim = os.path.join(CSRC, "dropin_evaluate.c")
    return _digest([fn, N, K, core_id, open(shim, "rb").read(), open(os.path.join(INCLUDE, "srbd_mpc.h"), "rb").read()])


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"build failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")


def _build_dropin_lib(fn: str, N: int, K: int | None, core: str, force: bool, verbose: bool) -> str:
    shim = os.path.join(CSRC, "dropin_evaluate.c")
    out = os.path.join(LIB_DIR, dropin_lib_name(fn, N, K))
    sid = _shim_hash(fn, N, K, embedded_id(core) or "")
    if not force and embedded_id(out) == sid:
        return out
    defs = ["-DSRBD_FN_FORMER"] if fn == "qp_former" else ["-DSRBD_FN_PDIPM", f"-DSRBD_ITERS={K}"]
    cmd = ["gcc", "-O2", "-fPIC", "-shared", f"-DSRBD_N={N}", *defs, f'-DSRBD_SHIM_ID="{sid}"', "-o", out, shim,
           f"-L{LIB_DIR}", "-lsrbd_mpc", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    _run(cmd)
    return out


def build_dropin(kind: str, N: int, K: int | None) -> str:
    """Thin CusADi-ABI library for one (function, horizon, iterations) configuration."""
    fn = "qp_former" if kind == "qp_former" else "sparse_pdipm_multiple_iterations"
    core = build()
    return _build_dropin_lib(fn, N, K, core, False, False)


# the HIP translation units of libsrbd_mpc.so and their unit-specific flags: the N = 20 register
# kernels in their own unit, scheduled with the register-pressure trackers (csrc/reg20.hpp)
HIP_UNITS = {
    "srbd_mpc.hip": [],
    "srbd_reg20.hip": ["-mllvm", "-amdgpu-use-amdgpu-trackers=1"],
    "srbd_regN.hip": ["-mllvm", "-amdgpu-use-amdgpu-trackers=1"],  # the other register horizons
    "srbd_backward.hip": [],  # the backward pass: adjoint KKT solve, QP-data gradients, former / prep / wrench VJPs
}


_COMMON_FLAGS = ["-O3", "-std=c++17"]


def unit_compile_cmd(unit: str, extra: list[str], csrc: str | None = None, replace: dict | None = None) -> list[str]:
    """hipcc command line of one translation unit exactly as the product build compiles it: the one
    constructor of a unit's command line, for the product, the variants (build_core) and the ISA
    listings (isa_listings). `csrc` is another source directory, `replace` maps a unit to the file
    compiled in its place."""
    src = (replace or {}).get(unit) or os.path.join(csrc or CSRC, unit)
    return [HIPCC, f"--offload-arch={ARCH}", *_COMMON_FLAGS, *HIP_UNITS[unit], *extra, src]


def _compile_parallel(cmds: list[list[str]]) -> None:
    """Run independent compiles at once and pass their diagnostics on; on any failure the others are
    killed and reaped before raising, so no orphan keeps writing objects into lib/."""
    procs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for c in cmds]
    failed = None
    try:
        for c, pr in zip(cmds, procs):
            out, err = pr.communicate()
            if pr.returncode != 0:
                failed = f"build failed: {' '.join(c)}\n{out}\n{err}"
                break
            sys.stderr.write(err)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
            pr.wait()
    if failed:
        raise RuntimeError(failed)


def build_core(out: str, csrc: str | None = None, flags=(), unit_flags: dict | None = None,
               replace: dict | None = None, objdir: str | None = None, force: bool = True,
               verbose: bool = False) -> dict[str, list[str]]:
    """Compile the units of HIP_UNITS with their flags and link them into `out`: the one recipe of
    libsrbd_mpc.so, for the product (build()) and for every variant (scripts/build_variant.py).
      csrc        source directory (default: the package's). A patched copy keeps the
                  biped_pympc_amd/csrc + include layout, as srbd_mpc.hip includes ../../include/srbd_mpc.h
      flags       extra flags for every unit, after the product's
      unit_flags  {unit: extra flags}, e.g. a force-included header that may go into one unit only
      replace     {unit: source file compiled in its place}
      objdir      where the objects go (default: a temporary directory). Unless `force`, an object there
                  is reused when its .id sidecar records the hash of exactly what it was compiled from
    The embedded build id is source_hash() of `csrc`, digested again with the extra flags and the
    replacements where there are any: only identical sources and flags give the product's id.
    Returns {unit: command line} of the units it compiled."""
    sources = core_sources(csrc)
    unit_flags, replace = unit_flags or {}, {u: os.path.abspath(f) for u, f in (replace or {}).items()}
    bid = source_hash(sources)
    if flags or unit_flags or replace:
        bid = _digest([bid, repr(list(flags)), repr(sorted(unit_flags.items())),
                       *[x for u, f in sorted(replace.items()) for x in (u, open(f, "rb").read())]])
    with tempfile.TemporaryDirectory() if objdir is None else contextlib.nullcontext(objdir) as od:
        # srbd_build_id() is defined in the main unit; the id names the sources and flags of all units
        objs = {u: os.path.join(od, u.replace(".hip", ".o")) for u in HIP_UNITS}
        cmds = {u: unit_compile_cmd(u, [*flags, *unit_flags.get(u, []), "-fPIC", "-c",
                                        *([f'-DSRBD_BUILD_ID="{bid}"'] if u == "srbd_mpc.hip" else []),
                                        "-o", o], csrc, replace) for u, o in objs.items()}
        ids = {u: _unit_hash(u, c, sources) for u, c in cmds.items()}
        stale = {u: c for u, c in cmds.items() if force or not (
            os.path.exists(objs[u]) and os.path.exists(objs[u] + ".id") and open(objs[u] + ".id").read().strip() == ids[u])}
        tmp = out + ".tmp"
        link = [HIPCC, f"--offload-arch={ARCH}", "-fPIC", "-shared", "-o", tmp, *objs.values()]
        for c in [*stale.values(), link] if verbose else []:
            print(" ".join(c))
        for u in stale:  # no sidecar describes an object while it is rewritten
            if os.path.exists(objs[u] + ".id"):
                os.remove(objs[u] + ".id")
        _compile_parallel(list(stale.values()))  # independent translation units
        for u in stale:
            with open(objs[u] + ".id", "w") as fh:
                fh.write(ids[u] + "\n")
        _run(link)
    os.replace(tmp, out)  # a process that has the old library mapped keeps its copy
    if embedded_id(out) != bid:
        raise RuntimeError(f"{out}: build id {embedded_id(out)} != {bid}")
    return stale


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(LIB_DIR, exist_ok=True)
    core = os.path.join(LIB_DIR, "libsrbd_mpc.so")
    bid = source_hash()
    if force or embedded_id(core) != bid:
        build_core(core, objdir=LIB_DIR, force=force, verbose=verbose)
        if embedded_id(core) != bid:
            raise RuntimeError(f"{core}: build id {embedded_id(core)} != source hash {bid}")
    for fn, N, K in DROPIN_CONFIGS:
        _build_dropin_lib(fn, N, K, core, force, verbose)
    return core


REGN_PARTS = 6  # csrc/srbd_regN.hip SRBD_REGN_PART: its horizons in six parts, for ISA listings


def isa_listings(outdir: str, units=None) -> dict[str, list[str]]:
    """Device ISA of the given units (default: all) as the product compiles them: {unit: .s files},
    srbd_regN.hip in its REGN_PARTS horizon parts, everything compiled concurrently."""
    outs, cmds = {}, []
    for u in HIP_UNITS if units is None else units:
        parts = [[f"-DSRBD_REGN_PART={k}"] for k in range(REGN_PARTS)] if u == "srbd_regN.hip" else [[]]
        outs[u] = [os.path.join(outdir, f"{u}.{k}.s") for k in range(len(parts))]
        cmds += [unit_compile_cmd(u, [*defs, "--cuda-device-only", "-S", "-o", o]) for defs, o in zip(parts, outs[u])]
    _compile_parallel(cmds)
    return outs


# ---- test-only primitive harness (tests/csrc/prim_harness.hip -> tests/libprim_harness.so) ----
# Not a product source: it lives outside csrc/, so core_sources(), source_hash() and the product
# libraries do not depend on it. tests/test_gpu_primitives.py loads it with ctypes.
PRIM_HARNESS_SRC = os.path.join(ROOT, "tests", "csrc", "prim_harness.hip")
PRIM_HARNESS_LIB = os.path.join(ROOT, "tests", "libprim_harness.so")
_PRIM_ID_RE = re.compile(rb"srbd-prim-id:([0-9a-f]{16})")


def prim_harness_hash() -> str:
    """Id of the primitive harness: sha256 over the harness source, every csrc/*.hpp it may include
    and the compile flags. The GPU tests fail when the library's embedded id differs from this."""
    parts = [ARCH, repr(_COMMON_FLAGS), "prim_harness.hip", open(PRIM_HARNESS_SRC, "rb").read()]
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hpp"):
            parts += [f, open(os.path.join(CSRC, f), "rb").read()]
    return _digest(parts)


def prim_harness_embedded_id(path: str = PRIM_HARNESS_LIB) -> str | None:
    try:
        with open(path, "rb") as fh:
            m = _PRIM_ID_RE.search(fh.read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def prim_harness_compile_cmd(extra: list[str]) -> list[str]:
    """hipcc command line of the harness with the product's architecture and common flags (the ISA
    audit of tests/test_prim_harness_isa.py appends --cuda-device-only -S)."""
    return [HIPCC, f"--offload-arch={ARCH}", *_COMMON_FLAGS, f"-I{CSRC}", *extra, PRIM_HARNESS_SRC]


def build_prim_harness(force: bool = False, verbose: bool = False) -> str:
    """Compile the test-only primitive harness in one hipcc call; reused while its embedded id
    matches prim_harness_hash()."""
    pid = prim_harness_hash()
    if force or prim_harness_embedded_id() != pid:
        tmp = PRIM_HARNESS_LIB + ".tmp"
        cmd = prim_harness_compile_cmd(["-fPIC", "-shared", f'-DSRBD_PRIM_ID="{pid}"', "-o", tmp])
        if verbose:
            print(" ".join(cmd))
        _run(cmd)
        os.replace(tmp, PRIM_HARNESS_LIB)
        if prim_harness_embedded_id() != pid:
            raise RuntimeError(f"{PRIM_HARNESS_LIB}: id {prim_harness_embedded_id()} != source hash {pid}")
    return PRIM_HARNESS_LIB


# ---- test-only harness of the column-split chain primitives (tests/csrc/prim_harness_split.hip ->
# tests/libprim_harness_split.so, loaded by tests/test_gpu_primitives_split.py): the same recipe ----
PRIM_SPLIT_SRC = os.path.join(ROOT, "tests", "csrc", "prim_harness_split.hip")
PRIM_SPLIT_LIB = os.path.join(ROOT, "tests", "libprim_harness_split.so")


def prim_harness_split_hash() -> str:
    parts = [ARCH, repr(_COMMON_FLAGS), "prim_harness_split.hip", open(PRIM_SPLIT_SRC, "rb").read()]
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hpp"):
            parts += [f, open(os.path.join(CSRC, f), "rb").read()]
    return _digest(parts)


def build_prim_harness_split(force: bool = False, verbose: bool = False) -> str:
    pid = prim_harness_split_hash()
    if force or prim_harness_embedded_id(PRIM_SPLIT_LIB) != pid:
        tmp = PRIM_SPLIT_LIB + ".tmp"
        cmd = [HIPCC, f"--offload-arch={ARCH}", *_COMMON_FLAGS, f"-I{CSRC}", "-fPIC", "-shared",
               f'-DSRBD_PRIM_ID="{pid}"', "-o", tmp, PRIM_SPLIT_SRC]
        if verbose:
            print(" ".join(cmd))
        _run(cmd)
        os.replace(tmp, PRIM_SPLIT_LIB)
        if prim_harness_embedded_id(PRIM_SPLIT_LIB) != pid:
            raise RuntimeError(f"{PRIM_SPLIT_LIB}: id {prim_harness_embedded_id(PRIM_SPLIT_LIB)} != source hash {pid}")
    return PRIM_SPLIT_LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    print(build_prim_harness(force=True, verbose=True))
    print(build_prim_harness_split(force=True, verbose=True))
