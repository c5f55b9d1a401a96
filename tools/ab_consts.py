"""bench.py with A/B module constants set first (the pieces that have no environment switch):

    python tools/ab_consts.py gate=0 merge=0 -- --gpus 1 --steps 20 --warmup 5

runs bench.py's main in this process after setting the named constants (0 / 1). Names:
  gate     depth_predictor_trans._GATE_AHEAD    the camera-parameter gate computed in camera prep
  gatekern cam_param_encoder._GATE_KERNEL       the gate as one kernel (off: the module chain, the parent's values)
  fuse     cam_param_encoder._FUSE_GATE_CONV    gate multiply + channel-last rows inside context_conv
  packed   depth_predictor_trans._PACKED_AHEAD  the correlation kernels' camera rows packed in camera prep
  query    depth_predictor_trans._NO_ZERO_QUERY the coarse layer without its zero query
  merge    uv_transformer._MERGE_PROJ           one GEMM for the fine layers' projections of the same rows
  cat      kernels._GEMM_CAT                    the MVT's mlp[0] reading [source | message] in place
  rows     kernels._ROWS_IN                     the DPT projects' 1x1 reading the token rows in place
  shuffle  kernels._SHUFFLE_OUT                 the DPT transposed convolutions' pixel shuffle in the 1x1's store
  tail     encoder_trans._DEFER_DA_TAIL         Depth-Anything's depth tail in the depth predictor's fork
"""
import importlib
import runpy
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NAMES = {
    "gate": ("transplat_amd.model.encoder.matching.depth_predictor_trans", "_GATE_AHEAD"),
    "gatekern": ("transplat_amd.model.utils.cam_param_encoder", "_GATE_KERNEL"),
    "fuse": ("transplat_amd.model.utils.cam_param_encoder", "_FUSE_GATE_CONV"),
    "packed": ("transplat_amd.model.encoder.matching.depth_predictor_trans", "_PACKED_AHEAD"),
    "query": ("transplat_amd.model.encoder.matching.depth_predictor_trans", "_NO_ZERO_QUERY"),
    "merge": ("transplat_amd.model.utils.uv_transformer", "_MERGE_PROJ"),
    "cat": ("transplat_amd.kernels", "_GEMM_CAT"),
    "rows": ("transplat_amd.kernels", "_ROWS_IN"),
    "shuffle": ("transplat_amd.kernels", "_SHUFFLE_OUT"),
    "tail": ("transplat_amd.model.encoder.encoder_trans", "_DEFER_DA_TAIL"),
}

if __name__ == "__main__":
    cut = sys.argv.index("--") if "--" in sys.argv else len(sys.argv)
    sys.path.insert(0, str(ROOT))
    for item in sys.argv[1:cut]:
        name, value = item.split("=")
        module, attr = NAMES[name]
        mod = importlib.import_module(module)
        if not hasattr(mod, attr):
            raise SystemExit(f"{module} has no {attr}")
        setattr(mod, attr, bool(int(value)))
    sys.argv = [str(ROOT / "bench.py"), *sys.argv[cut + 1:]]
    runpy.run_path(str(ROOT / "bench.py"), run_name="__main__")
