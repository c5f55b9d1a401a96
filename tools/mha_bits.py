"""One sha256 of the output bytes per dense-attention case, for comparing two builds of the library bit
for bit (TSPLAT_LIB points at the other build). The cases and their seeded inputs are the tests' own:
tests/test_encoder_ops.py's test_mha_kernel shapes x the three TSPLAT_MHA forms, test_mha_bias_folded,
test_mha_x3_kernel with and without bias, test_qkv_attention_cf_kernel; the presplit path on
tests/test_conv.py's test_gemm_x3_split_output_feeds_mha input; and tests/test_value_stress.py's MHA_SHAPES
(every form, the bias case, bf16x3) and CF_SHAPES x PATTERNS.

usage: [TSPLAT_LIB=other.so] python tools/mha_bits.py out.json"""
import hashlib
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import test_encoder_ops as TE  # noqa: E402
import test_value_stress as TV  # noqa: E402
from transplat_amd import kernels as K  # noqa: E402

dev = torch.device("cuda:0")
seeded = TE.seeded
FORMS = ("16", "16x8", "32")
out = {}


def params(fn, first):
    return next(m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0].startswith(first))


def put(tag, y):
    out[tag] = hashlib.sha256(y.contiguous().cpu().numpy().tobytes()).hexdigest()


def with_form(form):
    if form is None:
        os.environ.pop("TSPLAT_MHA", None)
    else:
        os.environ["TSPLAT_MHA"] = form


with torch.no_grad():
    for b, n, heads in params(TE.test_mha_kernel, "b,n,heads"):
        qkv = (seeded((b, n, 3 * heads * 64), 71) * 2.0).to(dev)
        for form in FORMS:
            with_form(form)
            put(f"mha {(b, n, heads)} form {form}", K.mha(qkv, heads, 64 ** -0.5, precision="fp32"))
    with_form(None)

    for b, n in params(TE.test_mha_bias_folded, "b,n"):
        qkv, bias = seeded((b, n, 3 * 12 * 64), 72) * 2.0, seeded((3 * 12 * 64,), 73) * 0.5
        put(f"mha bias {(b, n)}", K.mha(qkv.to(dev), 12, 64 ** -0.5, bias=bias.to(dev), precision="fp32"))

    for b, n, heads in params(TE.test_mha_x3_kernel, "b,n,heads"):
        qkv, bv = (seeded((b, n, 3 * heads * 64), 74) * 2.0).to(dev), (seeded((3 * heads * 64,), 75) * 0.5).to(dev)
        for bias in (False, True):
            put(f"mha x3 {(b, n, heads)} bias={bias}",
                K.mha(qkv, heads, 64 ** -0.5, bias=bv if bias else None, precision="bf16x3"))

    x = seeded((2, 325, 768), 211).to(dev)
    w = (seeded((2304, 768), 212) / 768 ** 0.5).to(dev)
    with K.dense_precision("bf16x3"):
        put("mha x3 presplit", K.mha_presplit(K.gemm_x3(x, w, seeded((2304,), 213).to(dev), act="split"), 12, 0.125))

    for case in params(TE.test_qkv_attention_cf_kernel, "vb,heads"):
        vb, heads, views, t = case
        put(f"cf {case}", K.qkv_attention_cf((seeded((vb, 3 * heads * 32, t), 81) * 2.0).to(dev), heads, views))

    for p in TV.PATTERNS:
        for n, heads, bias in [(n, h, False) for n, h in TV.MHA_SHAPES] + [(325, 2, True)]:
            qkv, bv = TV.mha_case(n, heads, p, bias)[:2]
            for form in FORMS:
                with_form(form)
                put(f"steered mha n={n} bias={bias} {p} form {form}",
                    K.mha(qkv.to(dev), heads, TV.MHA_SCALE, bias=bv.to(dev) if bias else None, precision="fp32"))
            with_form(None)
            if not bias:
                put(f"steered mha x3 n={n} {p}", K.mha(qkv.to(dev), heads, TV.MHA_SCALE, precision="bf16x3"))
        for shp in TV.CF_SHAPES:
            put(f"steered cf {shp} {p}", K.qkv_attention_cf(TV.cf_case(*shp, p)[0].to(dev), shp[1], shp[2]))

Path(sys.argv[1]).write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
print(f"{len(out)} cases -> {sys.argv[1]}")
