"""Alternating A/B of the one-launch controller step inside ONE process: an earlier library (A), the
product library with MPCConf.compute_cost off (B) and on (C). Both libraries are loaded side by side
and the three variants take turns, 8 rounds of 400 steps each with the order rotated per round, so
box drift hits all of them equally; HIP-event time per step (DESIGN.md 6b records the figures).
Run on the GPU box:  python scripts/objective_ab.py EARLIER_LIB [N ...]    (default N = 10 20)
Writes $OUT/objective_ab.json (OUT defaults to bench_out) and prints each round.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from biped_pympc_amd import _native  # noqa: E402
from biped_pympc_amd.utils.synthetic import make_controller  # noqa: E402

earlier = os.path.abspath(sys.argv[1])
horizons = [int(a) for a in sys.argv[2:]] or [10, 20]
B, K, ROUNDS, STEPS = 4096, 10, 8, 400

new_lib = _native.lib()
os.environ["SRBD_LIB"] = earlier  # _native.lib() binds an earlier build tolerantly (missing symbols raise on call)
_native._lib = None
old_lib = _native.lib()
del os.environ["SRBD_LIB"]
print("product", new_lib.srbd_build_id().decode(), "earlier", old_lib.srbd_build_id().decode(), flush=True)
assert new_lib.srbd_build_id() != old_lib.srbd_build_id(), "both handles name the same build"


def pct(a, b):
    d = (a - b) / b * 100
    return {"mean": float(d.mean()), "std": float(d.std(ddof=1)), "min": float(d.min()), "max": float(d.max()),
            "positive_rounds": int((d > 0).sum())}


result = {}
for N in horizons:
    variants = {}
    for name, lib, cost in (("earlier", old_lib, False), ("product", new_lib, False), ("product_cost", new_lib, True)):
        _native._lib = lib
        _native.prepare_device()
        c = make_controller(B, N, seed=3, device="cuda", n_iter=K)
        c.cfg.compute_cost = cost
        variants[name] = (lib, c)
    names = list(variants)

    def block(name, steps):
        lib, c = variants[name]
        _native._lib = lib
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s = torch.cuda.current_stream()
        e0.record(s)
        for _ in range(steps):
            c.run()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for name in names:
        block(name, 50)  # warm-up
    torch.cuda.synchronize()
    w = {n: variants[n][1].foot_wrench.clone() for n in names}  # same steps so far: the same wrench, bit for bit
    assert torch.equal(w["earlier"], w["product"]) and torch.equal(w["product"], w["product_cost"]), "wrench differs"
    assert not variants["product"][1].cost.any() and bool(variants["product_cost"][1].cost.any())
    times = {n: [] for n in names}
    for r in range(ROUNDS):
        for name in names[r % 3:] + names[:r % 3]:
            times[name].append(block(name, STEPS))
        print(f"N={N} round {r}: " + "  ".join(f"{n} {times[n][-1]:.4f}" for n in names), flush=True)
    t = {n: np.array(v) for n, v in times.items()}
    result[N] = {"ms": {n: [float(x) for x in v] for n, v in t.items()},
                 "mean_ms": {n: float(v.mean()) for n, v in t.items()},
                 "product_vs_earlier_pct": pct(t["product"], t["earlier"]),
                 "cost_on_vs_off_pct": pct(t["product_cost"], t["product"])}
    print(f"N={N}", json.dumps({k: v for k, v in result[N].items() if k != "ms"}), flush=True)
out = os.environ.get("OUT", os.path.join(ROOT, "bench_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "objective_ab.json"), "w") as fh:
    json.dump(result, fh, indent=1)
