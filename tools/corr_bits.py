"""One sha256 of the output bytes per correlation case, for comparing two builds of the library bit for
bit (TSPLAT_LIB points at the other build). The cases and their seeded inputs are the tests' own:
tests/test_corr_shapes.py's SHAPES, SWEEP and CONSTRUCTIONS x every coarse variant, CROSS_SHAPES, the
constructions and the one-hot case x CROSS_ROUTES, the test_msda_shapes cases through both entry points; and from
tests/test_encoder_ops.py msda_raw at the two map sizes of test_msda_raw_kernel and MSDA_CASES.

usage: [TSPLAT_LIB=other.so] python tools/corr_bits.py out.json"""
import hashlib
import importlib.util
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
spec = importlib.util.spec_from_file_location("test_corr_shapes", ROOT / "tests" / "test_corr_shapes.py")
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)
import test_encoder_ops as TE  # noqa: E402  (test_corr_shapes put tests/ on the path)
from transplat_amd import kernels as K  # noqa: E402

dev = torch.device("cuda:0")
seeded = T.seeded
KNOBS = sorted({k for env in T.COARSE_VARIANTS.values() for k in env})
out = {}


def params(fn, first):
    return next(m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0].startswith(first))


def put(tag, y):
    out[tag] = hashlib.sha256(y.contiguous().cpu().numpy().tobytes()).hexdigest()


def to_dev(ts):
    return [t.to(dev) for t in ts]


with torch.no_grad():
    for param in T.COARSE_CASES:
        case = param.values[0]
        (intr, pose, disp), (h, w, b) = T._case_cams(case)
        args = to_dev((seeded((b, 2, h * w, 128), 31), intr, pose, disp))
        for name, env in T.COARSE_VARIANTS.items():
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            put(f"coarse {param.id} {name}", K.uv_coarse(*args, h, w))
    for k in KNOBS:
        os.environ.pop(k, None)

    for param in T.CROSS_CASES:
        args, (h, w) = T._cross_inputs(param.values[0])
        args = to_dev(args)
        for route in T.CROSS_ROUTES:
            put(f"cross {param.id} {route}", T._cross_route(K, route, args, h, w))

    for h, w in params(T.test_msda_shapes, "hw"):
        for points in params(T.test_msda_shapes, "points"):
            n, q = 2, 37
            value, loc = seeded((n, h * w, 128), 51), T._msda_locations(n, q, points, h, w)
            wts = torch.softmax(seeded((n, q, points), 53), -1)
            for entry in params(T.test_msda_shapes, "entry"):
                put(f"msda {h}x{w} P={points} {entry}", T._msda_entry(K, entry, *to_dev((value, loc, wts)), h, w))

    for h, w in params(TE.test_msda_raw_kernel, "hw"):
        ow = torch.zeros((2, h * w, 128))
        ow[..., :8] = seeded((2, h * w, 8), 55) * 3.0
        ow[..., 8:12] = seeded((2, h * w, 4), 56)
        put(f"msda_raw {h}x{w}", K.msda_raw(seeded((2, h * w, 128), 54).to(dev), ow.to(dev), 4, h, w))

    for i, case in enumerate(TE.MSDA_CASES):
        put(f"ms_deform_attn case {i}", K.ms_deform_attn(*to_dev(TE._msda_case(*case, seed=81))))

Path(sys.argv[1]).write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
print(f"{len(out)} cases -> {sys.argv[1]}")
