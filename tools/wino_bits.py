"""One sha256 of the output bytes per Winograd case of tests/test_conv.py, for comparing two builds of
the library bit for bit (TSPLAT_LIB points at the other build). The cases and their seeded inputs are
the tests' own: WINO_CASES and the extra bf16x3 shapes, the relu-in / residual shapes, the persistent
walk and the fused every-form case; fp32 with TSPLAT_WINO_WG / KS auto and forced, bf16x3 over
TSPLAT_WINO3_FORM auto, 1-6 x TSPLAT_WINO3_STAGE auto, 0.

usage: [TSPLAT_LIB=other.so] python tools/wino_bits.py out.json"""
import hashlib
import importlib.util
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
spec = importlib.util.spec_from_file_location("test_conv", ROOT / "tests" / "test_conv.py")
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)
from transplat_amd import kernels as K  # noqa: E402

K._FEW = False  # the Winograd kernels, as the tests pin them
dev = torch.device("cuda:0")
seeded = T.seeded
KNOBS = ("TSPLAT_WINO_WG", "TSPLAT_WINO_KS", "TSPLAT_WINO3_FORM", "TSPLAT_WINO3_STAGE", "TSPLAT_WINO3_PWG")
out = {}


def params(fn, first):
    return next(m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0].startswith(first))


def run(name, env, fn):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    y = fn().contiguous().cpu()
    tag = name + " " + " ".join(f"{k[7:]}={v}" for k, v in sorted(env.items()))
    out[tag.strip()] = hashlib.sha256(y.numpy().tobytes()).hexdigest()


def x3_envs():
    for form in ("auto", "1", "2", "3", "4", "5", "6"):
        for stage in ("auto", "0"):
            env = {}
            if form != "auto":
                env["TSPLAT_WINO3_FORM"] = form
            if stage != "auto":
                env["TSPLAT_WINO3_STAGE"] = stage
            yield env


with torch.no_grad():
    for case in params(T.test_conv3x3_wino_bf16x3_kernel, "n,ci"):
        n, ci, co, h, w, bias, act = case
        x = seeded((n, ci, h, w), 41).to(dev)
        wt = (seeded((co, ci, 3, 3), 42) * (1.0 / (9 * ci) ** 0.5)).to(dev)
        b = seeded((co,), 43).to(dev) if bias else None
        if case in T.WINO_CASES:
            for wg in ("auto", "32", "32x2", "64"):
                env = {} if wg == "auto" else {"TSPLAT_WINO_WG": wg[:2], "TSPLAT_WINO_KS": "2" if wg == "32x2" else "1"}
                run(f"fp32 {case}", env, lambda: K.conv3x3_wino(x, wt, b, act, precision="fp32"))
        for env in x3_envs():
            run(f"x3 {case}", env, lambda: K.conv3x3_wino(x, wt, b, act, precision="bf16x3"))

    for case in params(T.test_conv3x3_wino_bf16x3_relu_in_residual, "n,c"):
        n, c, h, w, skip = case
        x = seeded((n, c, h, w), 91).to(dev)
        wt = (seeded((c, c, 3, 3), 92) * (1.0 / (9 * c) ** 0.5)).to(dev)
        b = seeded((c,), 93).to(dev)
        sk = seeded((n, c, h, w), 94).to(dev) if skip else None
        for env in x3_envs():
            run(f"relu_in {case}", env, lambda: K.conv3x3_wino(x, wt, b, precision="bf16x3", residual=x, residual2=sk,
                                                              relu_in=True))

    for chans in params(T.test_conv3x3_wino_bf16x3_persistent_walk, "chans"):
        ci = sum(chans)
        parts = [seeded((3, c, 40, 72), 120 + c + 7 * i).to(dev) for i, c in enumerate(chans)]
        wt = (seeded((48, ci, 3, 3), 131) * (1.0 / (9 * ci) ** 0.5)).to(dev)
        b = seeded((48,), 132).to(dev)
        r1, r2 = seeded((3, 48, 40, 72), 133).to(dev), seeded((3, 48, 40, 72), 134).to(dev)
        for wgs in params(T.test_conv3x3_wino_bf16x3_persistent_walk, "wgs"):
            run(f"walk {chans}", {"TSPLAT_WINO3_FORM": "5", "TSPLAT_WINO3_PWG": wgs},
                lambda: K.conv3x3_wino(parts[0], wt, b, "gelu", extra=(parts[1],), precision="bf16x3", residual=r1,
                                       residual2=r2, relu_in=True))

    c = {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in T._fused_every_form_case().items()}
    for env in x3_envs():
        run("fused", env, lambda: K.conv3x3_wino(c["parts"][0], c["wt"], c["b"], "gelu", extra=(c["parts"][1],),
                                                 precision="bf16x3", residual=c["r1"], residual2=c["r2"], relu_in=True))

for k in KNOBS:
    os.environ.pop(k, None)
Path(sys.argv[1]).write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
print(f"{len(out)} cases -> {sys.argv[1]}")
