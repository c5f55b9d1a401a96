#!/usr/bin/env python3
"""Benchmark: novel views/s at 256x256 with 2 context views on MI355X (BASELINE.json metric).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 launched by
torch.distributed.run, one rank per GPU. W untimed warm-up steps, then exactly K steps between a
barrier + device synchronise on both sides; the slowest rank's time is used; rank 0 prints ONE
JSON line.

Workloads (a "step" = one pass of the hot path over one batch of synthetic scenes):
  e2e    : encoder (backbone + DA-V2 + depth predictor + adapter) -> decoder for B scenes of
           2 context views, rendering 3 target views each (reference test_step,
           src/model/model_wrapper.py:185-323, metrics excluded)
  raster : the decoder alone on precomputed synthetic Gaussians (G = 131,072 per scene)
Scenes shard embarrassingly across ranks (rank r renders its own B scenes; no data-path
collective); one all-reduce of the timing and a gather of per-rank counts close the run.

Self-launch: `python bench.py --gpus N` with N > 1 and no torch.distributed environment starts
`torch.distributed.run --nproc-per-node N` itself (as a child process, before anything touches the
GPU) and exits with its status; under a launcher, --gpus must equal WORLD_SIZE or the run fails.
`--workload selftest` is a CPU-only stand-in step (no GPU, no kernels) that exercises exactly
this launch / barrier / max-over-ranks / JSON path (tests/test_distributed.py).

A plain run does only what the headline figure needs: set-up, the warm-up steps, the K timed steps,
the output dump if `--dump-outputs DIR` is given, and the result line (metric, value, unit,
ms_per_step, dtype, config). `--full` adds everything else the result line can carry, each measured
in passes of its own after the timed region: the roofline objects (dominant kernel, Winograd
convolutions, split-bf16 GEMMs, the render kernel's VALU roofline), the committed PMC traffic
digest, the launched-routes label of the workload string and the CPU baseline. The options that
only shape those (--dominant, --no-cpu-baseline, --cpu-baseline-seconds, --cpu-baseline-1thread) are
accepted and unused in a plain run, whose `config.workload` ends after the precision modes.

`--dump-outputs DIR` writes what the last timed step returned to its caller as DIR/<name>.npy
(float32; `color` for e2e, `color` and `radii` for raster, `out` for selftest; rank r > 0 writes
<name>.rank<r>.npy). Inputs and weights are seeded, so two builds run with the same arguments can
be compared output for output. Above 64 MiB on disk, a fixed seeded sample of each array is written.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import subprocess
import sys
import time
from pathlib import Path

import torch
import torch.distributed as dist

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md chip table)
FP32_MFMA_PEAK_TFS = 157.3  # v_mfma_f32_16x16x4_f32 dense peak (= FP32 vector peak)
BF16_MFMA_PEAK_TFS = 2500.0  # dense bf16 MFMA peak (no 2:1 sparsity), MI355X_MICROARCH.md
RASTER_BYTES_PER_VIEW = None  # computed: G*(12+24+4*d_sh*3+4) + H*W*12


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=["e2e", "raster", "selftest"], default="e2e")
    ap.add_argument("--dense-dtype", choices=["bf16x3", "fp32", "bf16"], default="bf16x3",
                    help="dense convs / GEMMs: bf16x3 = split-bf16 products with fp32 accumulation (the "
                         "stand-in for the reference's TF32, src/main.py:15; more precise than it), fp32 = "
                         "exact fp32, bf16 = autocast (narrower than the reference)")
    ap.add_argument("--attn-dtype", choices=["auto", "fp32", "bf16x3", "bf16"], default="auto",
                    help="window attention: auto = bf16 under bf16 dense layers, bf16x3 (split-bf16 products, "
                         "fp32 softmax) under bf16x3 ones, else exact fp32")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need, after the timed steps: roofline "
                         "objects (per-kernel HIP-event passes), PMC traffic digest, launched-routes label, CPU "
                         "baseline. Off by default: a plain run times the steps and prints the result line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the arrays the last timed step returned as DIR/<name>.npy "
                         "(float32, at most 64 MB in all: a fixed seeded sample of anything larger)")
    ap.add_argument("--dominant", default=None, help="kernel timed for the roofline object (--full)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of one hipGraph per step")
    ap.add_argument("--batch", type=int, default=1, help="scenes per step per GPU")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=15.0, help="with --full: its time budget")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--cpu-baseline-1thread", action="store_true",
                    help="with --full: also time the e2e CPU port on ONE thread (one full scene: several minutes)")
    ap.add_argument("--no-conv-search", action="store_true",
                    help="MIOpen's default convolution algorithm choice instead of its measured search "
                         "(torch.backends.cudnn.benchmark, on by default: +2.4%% e2e at b = 1)")
    ap.add_argument("--conv-deterministic", action="store_true",
                    help="only MIOpen's run-to-run deterministic solvers (torch.backends.cudnn.deterministic). "
                         "A no-op for the bf16x3 default since round 5: no convolution of that step reaches "
                         "MIOpen (tests/test_conv.py::test_encoder_runs_no_library_convolution) and its outputs "
                         "are bit-identical run to run (tools/determinism_probe.py). Other modes still route "
                         "convolutions to MIOpen, whose deterministic choices collapse exact-fp32 C2 (22.8 "
                         "views/s) and the bf16-dense C3 variant (53.4): profiles/r4/final_det/")
    return ap.parse_args()


def self_launch(args) -> int | None:
    """--gpus N > 1 without a launcher: run this script under torch.distributed.run with N local
    ranks (a child process; this one has not touched the GPU) and return its exit status. Under a
    launcher, a --gpus that disagrees with WORLD_SIZE is an error (the JSON would misreport)."""
    world = os.environ.get("WORLD_SIZE")
    if world is not None:
        if args.gpus != int(world):
            raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
        return None
    if args.gpus <= 1:
        return None
    import socket

    with socket.socket() as sk:  # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={port}", str(Path(__file__).resolve()), *sys.argv[1:]]
    return subprocess.call(cmd)


def init_dist():
    """One process per GPU (torch.distributed.run env). RCCL ("nccl") by default; the rehearsal
    override TSPLAT_DIST_BACKEND=gloo (with LOCAL_RANK folded onto the visible GPUs) lets the N > 1
    path run on a single-GPU box — the timing all-reduce is the only collective either way."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("TSPLAT_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl" or torch.cuda.device_count() > 0:
            torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
        else:
            dist.init_process_group(backend)
    return world, rank, local


def timed_steps(step, steps: int, world: int, sync, device) -> float:
    """EXACTLY `steps` calls of `step` bracketed by sync + barrier on both sides; the MAX of the
    ranks' wall times (every rank returns the same value). `sync` waits for the device
    (torch.cuda.synchronize on the GPU). The only collectives are the barriers and this one
    all-reduce of a scalar (RCCL on GPUs, gloo in the CPU tests)."""
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def raster_bytes_per_view(g: int, d_sh: int, h: int, w: int) -> int:
    # means 12 + cov 24 (upper triangle of the 3x3) + SH 3*d_sh*4 + opacity 4, image 3*4 per pixel
    return g * (12 + 24 + 3 * d_sh * 4 + 4) + h * w * 12


def build_raster_workload(batch: int, device, scene_offset: int):
    from transplat_amd import synthetic as S
    from transplat_amd.model.decoder.hip_splatting import prepare_cameras, rasterize

    hw = (256, 256)
    g = S.make_gaussians(batch, image_shape=hw, scene_offset=scene_offset, device=device)
    tb = S.make_batch(batch, image_shape=hw, scene_offset=scene_offset, device=device)["target"]
    b, v = tb["near"].shape
    cams = prepare_cameras(tb["extrinsics"].reshape(b * v, 4, 4), tb["intrinsics"].reshape(b * v, 3, 3),
                           tb["near"].reshape(-1), tb["far"].reshape(-1), torch.zeros(b * v, 3, device=device))

    def step():
        return rasterize(g["means"], g["covariances"], g["harmonics"], g["opacities"], cams, hw, v,
                         check=False)

    g_per_scene = g["means"].shape[1]
    info = {
        "views_per_step": b * v,
        "dominant": "raster",
        "alg_bytes_per_launch": raster_bytes_per_view(g_per_scene, g["harmonics"].shape[-1], *hw) * b * v,
        "workload": "raster-only: decoder on synthetic Gaussians (G=131072/scene, 3 target views)",
    }

    def cpu_inputs():  # host copies for the CPU baseline (--full), made only when asked for
        return {k: t.cpu() for k, t in g.items()}, cams.to("cpu"), hw, v

    return step, info, cpu_inputs


# blend VALU per (entry, 8x8 block) of the render kernel: one wave64 instruction per (entry, pixel)
# step -- dx, dy, the power's Horner form (3 mul + 2 fma), exp2, o * e, min 0.99, the three decisions
# (2 compares + the test_T fma and compare), w = alpha T and its select, 3 colour fmas, the T select:
# 20, counted in the gfx950 ISA of the quad loop (81 VALU per 4 entries, csrc/raster.hip render_kernel)
RENDER_VALU_PER_ENTRY = 20
# wave64 VALU issue: 32 lanes per clock per SIMD (157.3 TFLOP/s fp32 FMA = 1024 SIMDs x 64 FLOP/clk x 2.4 GHz)
VALU_PEAK_TLANE_OPS = 1024 * 32 * 2.4e9 / 1e12


def render_valu_roofline(step, n_prof: int) -> dict:
    """The render kernel against its VALU roofline (what bounds it; HBM is far off): entry-pixel
    evaluations per launch (the diag-5 counters: entries each 8x8-block wave blended) x the blend's
    VALU per evaluation / the render kernel's average duration (HIP events), against the gfx950
    VALU issue peak. Measured outside the timed region."""
    from transplat_amd import _lib

    _lib.prof_enable("raster_render")
    for _ in range(n_prof):
        step()
    ms, launches = _lib.prof_read()
    _lib.prof_enable(None)
    os.environ["TSPLAT_RASTER_DIAG"] = "5"
    try:
        color = step()[0]
        torch.cuda.synchronize()
    finally:
        os.environ["TSPLAT_RASTER_DIAG"] = "0"
    # diag 5 writes (cycles, entries, chunks) of the wave into each pixel of its 8x8 block
    c = color.reshape(-1, 3, color.shape[-2] // 8, 8, color.shape[-1] // 8, 8)[:, :, :, 0, :, 0].double()
    entries, chunks = float(c[:, 1].sum()), float(c[:, 2].sum())
    avg_ms = ms / launches
    evals = entries * 64
    achieved = evals * RENDER_VALU_PER_ENTRY / (avg_ms * 1e-3) / 1e12
    cyc = c[:, 0].flatten()
    return {"kernel": "raster_render", "bound": "valu", "achieved": achieved, "peak": VALU_PEAK_TLANE_OPS,
            "unit": "T lane-ops/s", "frac": achieved / VALU_PEAK_TLANE_OPS, "avg_launch_ms": avg_ms,
            "entry_pixel_evals_per_launch": evals, "valu_per_eval": RENDER_VALU_PER_ENTRY,
            "chunks_per_launch": chunks,
            "wave_cycles_p50_max": [float(cyc.median()), float(cyc.max())]}


def committed_traffic(kernel: str, dense_dtype: str, batch: int):
    """HBM traffic per launch of `kernel` from the newest committed PMC digest
    (profiles/<round>/traffic_<kernel>_<dtype>_b<batch>.json, written by tools/pmc_traffic.py from
    separate rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this same workload), or None."""
    root = Path(__file__).resolve().parent / "profiles"
    name = f"traffic_{kernel}_{dense_dtype}_b{batch}.json"
    for d in sorted((p for p in root.glob("*") if p.is_dir()), reverse=True):
        f = d / name
        if f.exists():
            return json.loads(f.read_text())["traffic_bytes_per_launch"], str(f.relative_to(root.parent))
    return None, None


def e2e_roofline_info(kernel: str, batch: int, attn_dtype: str = "fp32") -> dict:
    """Algorithmic HBM bytes (or FLOPs) per launch of the hand-written encoder kernels at 256x256,
    2 views, D = 128, C = 128, per SURVEY §8d (units per launch = `batch` scenes)."""
    hw, c, d, p = 64 * 64, 128, 128, 4
    n = 2 * batch  # (b v) query maps per launch
    if kernel == "uv_cross":
        # value (other view) + key + offsets + logits + output, fp32, each read once
        per = n * hw * (c * 4 + c * 4 + d * p * 2 * 4 + d * p * 4 + d * 4)
        return {"dominant": kernel, "alg_bytes_per_launch": per, "bound": "hbm"}
    if kernel == "uv_cross_table":
        # the [HW, HW] correlation table + offsets + logits + output, each read / written once
        per = n * hw * (hw * 4 + d * p * 2 * 4 + d * p * 4 + d * 4)
        return {"dominant": kernel, "alg_bytes_per_launch": per, "bound": "hbm"}
    if kernel == "uv_coarse":
        per = n * hw * (c * 4 + d * 4) + n * hw * c * 4  # own + other features, output
        return {"dominant": kernel, "alg_bytes_per_launch": per, "bound": "hbm"}
    if kernel == "win_attn":
        # 4 L S d FLOPs per window, 8 windows per scene-call (v = 2). fp32: exact fp32 MFMA, priced
        # against the fp32 MFMA peak; bf16: the bf16-MFMA kernel, against the dense bf16 peak; bf16x3:
        # three bf16 MFMA products per fp32 product (hi*hi + hi*lo + lo*hi), so the MFMA work is 3x
        # the algorithmic FLOPs, priced against the dense bf16 peak (its fp32-equivalent rate is
        # reported beside it)
        flops = 4 * 1024 * 1024 * 128 * 8 * batch
        if attn_dtype == "bf16x3":
            return {"dominant": kernel, "alg_flops_per_launch": 3 * flops, "fp32_equivalent_flops_per_launch": flops,
                    "bound": "mfma", "peak_tflops": BF16_MFMA_PEAK_TFS,
                    "flops_note": "bf16 MFMA products: 3 x 4 L S d per window (split-bf16 hi*hi + hi*lo + lo*hi)"}
        return {"dominant": kernel, "alg_flops_per_launch": flops, "bound": "mfma",
                "peak_tflops": BF16_MFMA_PEAK_TFS if attn_dtype == "bf16" else FP32_MFMA_PEAK_TFS}
    if kernel == "raster":
        return {"dominant": kernel, "alg_bytes_per_launch": raster_bytes_per_view(131072, 25, 256, 256) * 3 * batch,
                "bound": "hbm"}
    raise ValueError(kernel)


def cpu_model() -> str:
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def cpu_baseline_e2e(model, seconds: float, one_thread: bool = False):
    """The same test_step on the host: the build's modules with the oracle's CPU restatements in
    place of the HIP kernels and the C oracle rasterizer (kind 'port'), on >= 1 scene. Torch and the
    rasterizer's OpenMP both use torch.get_num_threads() threads (the process's CPU share: 16 on
    the GPU box, where OMP_NUM_THREADS is set by the pool)."""
    import copy

    from oracle import encoder_ops as E
    from oracle import raster as oracle_raster
    from transplat_amd import kernels
    from transplat_amd import synthetic as S
    from transplat_amd.model.decoder.hip_splatting import prepare_cameras

    saved = {n: getattr(kernels, n) for n in E.KERNEL_RESTATEMENTS}
    for n in saved:
        setattr(kernels, n, getattr(E, n))
    threads = torch.get_num_threads()

    from transplat_amd.misc.benchmarker import Benchmarker

    bm = Benchmarker()  # the reference's stage tags, wall time per stage (CPU: no device sync)

    def run(budget, nthreads):
        torch.set_num_threads(nthreads)
        oracle_raster.set_threads(nthreads)
        t_raster, n_views, t0 = 0.0, 0, time.perf_counter()
        while True:
            batch = S.make_batch(1, image_shape=(256, 256))
            with torch.no_grad():
                g = enc(batch["context"], 0, deterministic=True, benchmarker=bm)
            t = batch["target"]
            cams = prepare_cameras(t["extrinsics"][0], t["intrinsics"][0], t["near"][0], t["far"][0], torch.zeros(3, 3))
            tr = time.perf_counter()
            oracle_raster.render(g.means, g.covariances, g.harmonics, g.opacities, cams, (256, 256), 3, 3)
            t_raster += time.perf_counter() - tr
            n_views += 3
            el = time.perf_counter() - t0
            if el >= budget:
                return n_views, el, t_raster

    try:
        enc = copy.deepcopy(model.encoder).float().cpu()
        enc.cfg.dense_dtype = "fp32"
        enc.cfg.attn_dtype = "fp32"
        n_views, el, t_raster = run(seconds, threads)
        stages = {tag: sum(ts) / len(ts) for tag, ts in bm.execution_times.items()}
        one = run(0.0, 1) if one_thread else None  # one full scene on one thread
    finally:
        torch.set_num_threads(threads)
        oracle_raster.set_threads(threads)
        for n, f in saved.items():
            setattr(kernels, n, f)
    res = {
        "value": n_views / el, "unit": "views/s", "cores": threads, "kind": "port",
        "sample": f"{n_views // 3} scene(s) x 3 views, 256x256: the build's encoder modules on CPU (torch, "
                  f"{threads} threads) with oracle/encoder_ops.py restatements for the HIP kernels + "
                  f"oracle/raster_ref.c (literal mode; OpenMP, {threads} threads; raster "
                  f"{t_raster / n_views * 1e3:.0f} ms/view), {el:.1f} s, host {cpu_model()}, nproc={os.cpu_count()}",
    }
    # per-stage seconds per scene of the port, and the like-for-like comparison with the reference's
    # own CPU path as measured in the survey container (backbone + depth predictor
    # only -- DA-V2, the e3nn adapter and the CUDA-only rasterizer do not run on the reference's CPU path)
    keep = ("encoder_2_backbone", "encoder_3_depth_anything", "encoder_4_depth_predictor", "encoder_5_gaussian_adapter",
            "encoder_4b_cost_volume_matching")
    res["stages_s_per_scene"] = {k: round(stages[k], 3) for k in keep if k in stages}
    res["stages_s_per_scene"]["raster_3_views"] = round(t_raster / (n_views // 3), 3)
    bb_dp = stages.get("encoder_2_backbone", 0.0) + stages.get("encoder_4_depth_predictor", 0.0)
    res["reference_cpu"] = {
        "backbone_plus_depth_predictor_s_per_scene": 5.24, "port_same_stages_s_per_scene": round(bb_dp, 3),
        "cores": 8, "kind": "reference",
        "sample": "the reference's own BackboneMultiview + DepthPredictorTrans, b = 1, 256x256, fp32, 8 torch "
                  "threads on the survey container's 8 Xeon vCPUs (BASELINE.md §2; reference code cannot run on "
                  "the GPU box). DA-V2 (weights / cv2 absent), the e3nn adapter and the rasterizer (CUDA-only "
                  "fork) have no runnable reference CPU path, so the full-step CPU figure is the port's.",
    }
    if one is not None:
        res["value_1thread"] = one[0] / one[1]
        res["sample"] += (f"; 1 thread: one scene in {one[1]:.1f} s = {one[0] / one[1]:.4f} views/s "
                          f"(raster {one[2] / one[0] * 1e3:.0f} ms/view)")
    return res


def cpu_baseline_raster(cpu_inputs, seconds: float):
    """Oracle C rasterizer on as many views as fit `seconds` (>= 1), with OpenMP over tiles at
    torch.get_num_threads() threads; a single-thread pass on a quarter of the budget is reported
    beside it."""
    from oracle import raster as oracle_raster

    g, cams, hw, vps = cpu_inputs
    one = {k: t[:1] for k, t in g.items()}
    deg = min(3, int(round(one["harmonics"].shape[-1] ** 0.5)) - 1)

    def run(budget):
        n_views, t0 = 0, time.perf_counter()
        while True:
            i = n_views % vps
            sub = type(cams)(*(getattr(cams, f)[i : i + 1] for f in cams.__dataclass_fields__))
            oracle_raster.render(one["means"], one["covariances"], one["harmonics"], one["opacities"], sub, hw, 1, deg)
            n_views += 1
            el = time.perf_counter() - t0
            if el >= budget:
                return n_views, el

    threads = torch.get_num_threads()
    oracle_raster.set_threads(1)
    n1, el1 = run(seconds / 4)
    oracle_raster.set_threads(threads)
    n_views, el = run(seconds)
    return {
        "value": n_views / el,
        "unit": "views/s",
        "cores": threads,
        "kind": "port",
        "value_1thread": n1 / el1,
        "sample": f"{n_views} views of one synthetic 256x256 scene (G=131072) through oracle/raster_ref.c "
                  f"(OpenMP over Gaussians / tiles, {threads} threads; 1 thread: {n1 / el1:.2f} views/s), "
                  f"{el:.1f} s, host {cpu_model()}, nproc={os.cpu_count()}",
    }


def keeping_last(step):
    """`step` wrapped to keep what its latest call returned (--dump-outputs): (wrapped, [last])."""
    last = [None]

    def timed():
        last[0] = step()

    return timed, last


def selftest_main(args, world, rank):
    """CPU stand-in step (a small matmul, plus rank-dependent sleep so the max-over-ranks is
    observable): the launch, barrier, timing all-reduce and JSON line of the real bench, no GPU.
    --dump-outputs writes the step's product as `out`; there is nothing for --full to add."""
    x = torch.randn(128, 128, generator=torch.Generator().manual_seed(rank))

    def step():
        time.sleep(0.01 * (rank + 1))
        return x @ x

    timed, last = keeping_last(step) if args.dump_outputs else (step, None)
    for _ in range(args.warmup):
        timed()
    elapsed = timed_steps(timed, args.steps, world, lambda: None, torch.device("cpu"))
    if args.dump_outputs:
        dump_outputs(last[0], Path(args.dump_outputs), rank)
    if rank == 0:
        print(json.dumps({"metric": "selftest steps/s", "value": world * args.steps / elapsed, "unit": "steps/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                          "config": {"workload": "selftest (CPU)", "parallelism": f"scene-shard x{world}"}}),
              flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    args = parse()
    rc = self_launch(args)
    if rc is not None:
        sys.exit(rc)
    world, rank, local = init_dist()
    if args.workload == "selftest":
        return selftest_main(args, world, rank)
    device = torch.device(f"cuda:{local}")
    torch.cuda.set_device(device)
    from transplat_amd.kernels import auto_attention

    attn_dtype = args.attn_dtype if args.attn_dtype != "auto" else auto_attention(args.dense_dtype)
    if args.workload == "raster":
        dtype_label = "fp32"
    else:
        dtype_label = {"bf16x3": "fp32 (bf16x3 dense, >= TF32)", "fp32": "fp32",
                       "bf16": "bf16 dense (narrower than the reference's TF32)"}[args.dense_dtype]
        dtype_label += f" + {attn_dtype} attention + fp32 raster"
    if not args.no_conv_search:
        torch.backends.cudnn.benchmark = True
    torch.backends.cudnn.deterministic = args.conv_deterministic
    from transplat_amd import _lib

    _lib.load()

    if args.workload == "raster":
        step, info, cpu_inputs = build_raster_workload(args.batch, device, scene_offset=rank * args.batch)
    else:
        from transplat_amd.e2e import build_e2e_workload

        step, info, model = build_e2e_workload(args.batch, device, scene_offset=rank * args.batch,
                                               dense_dtype=args.dense_dtype, graph=not args.no_graph,
                                               attn_dtype=args.attn_dtype, routes=args.full)
        info.update(e2e_roofline_info(args.dominant or "win_attn", args.batch, attn_dtype))
    if args.dominant and args.workload == "raster":
        info["dominant"] = args.dominant

    timed, last = keeping_last(step) if args.dump_outputs else (step, None)
    for _ in range(args.warmup):
        timed()
    elapsed = timed_steps(timed, args.steps, world, torch.cuda.synchronize, device)
    from transplat_amd.model.decoder.hip_splatting import check_status

    check_status(device)  # any capacity overflow during the timed steps invalidates the run
    if args.dump_outputs:  # before anything else launches: a graphed step's outputs are static buffers
        torch.cuda.synchronize()
        dump_outputs(last[0], Path(args.dump_outputs), rank)

    views = world * info["views_per_step"] * args.steps
    result = {
        "metric": "novel views/sec at 256x256, 2 ctx views; PSNR parity vs reference",
        "value": views / elapsed,
        "unit": "views/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": dtype_label,
        "data": "synthetic",
        "config": {
            "workload": info["workload"],
            "scenes_per_gpu_per_step": args.batch,
            "views_per_scene": 3,
            "image": [256, 256],
            "parallelism": f"scene-shard x{world}",
        },
    }
    if args.full:
        result.update(full_measurements(args, step, info, elapsed, attn_dtype))
        if rank == 0 and not args.no_cpu_baseline:
            if args.workload == "raster":
                result["cpu_baseline"] = cpu_baseline_raster(cpu_inputs(), args.cpu_baseline_seconds)
            else:
                result["cpu_baseline"] = cpu_baseline_e2e(model, args.cpu_baseline_seconds, args.cpu_baseline_1thread)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


DUMP_BUDGET_BYTES = 64 * 2**20  # of the .npy files on disk, headers included
NPY_HEADER_BYTES = 128  # numpy.save's header for a one-dimensional array (format 1.0, padded to 64)


def dump_outputs(out, folder: Path, rank: int = 0) -> None:
    """What one call of the timed path hands its caller, as <name>.npy in float32 (float64 for
    64-bit values): the decoder's `color` [b, v, 3, h, w] (and `depth` when it renders one) for the
    e2e step, `color` and the per-Gaussian `radii` for the raster-only step. Above DUMP_BUDGET_BYTES
    on disk, each array is cut to its share of the budget: the flattened array is split into equal
    strata and one element of each is kept, at an offset drawn from numpy's default_rng(0), so the
    sample is sorted, free of duplicates and the same for every run of the same shapes."""
    import numpy as np

    if torch.is_tensor(out):
        named = {"out": out}
    elif isinstance(out, tuple):
        named = dict(zip(("color", "radii"), out))
    else:
        named = {"color": out.color, "depth": out.depth}
    arrays = {}
    for name, t in named.items():
        if t is None:
            continue
        wide = t.dtype in (torch.float64, torch.int64)
        arrays[name] = t.detach().to("cpu", torch.float64 if wide else torch.float32).numpy()
    total = sum(a.nbytes for a in arrays.values())
    folder.mkdir(parents=True, exist_ok=True)
    payload = DUMP_BUDGET_BYTES - NPY_HEADER_BYTES * len(arrays)
    for name, a in arrays.items():
        if total > payload:
            keep = max(1, int(a.size * payload / total))  # a.nbytes * payload / total bytes of it
            lo = np.arange(keep, dtype=np.int64) * a.size // keep
            hi = np.append(lo[1:], a.size)
            a = a.reshape(-1)[lo + np.random.default_rng(0).integers(0, hi - lo)]
        np.save(folder / (f"{name}.npy" if rank == 0 else f"{name}.rank{rank}.npy"), a)


def full_measurements(args, step, info, elapsed, attn_dtype) -> dict:
    """--full: the roofline objects of the result line, measured after the timed region in passes
    of their own (HIP events around one kernel family at a time)."""
    from transplat_amd import _lib

    # dominant-kernel timing (HIP events on the launch stream), separate from the timed region;
    # event records cannot live inside a replayed hipGraph, so this pass launches eagerly (the
    # kernel and its inputs are the same). The encoder's concurrent Depth-Anything branch is
    # serialised for it, so a kernel's duration is its own, not shared with the other branch.
    prof_step = info.get("eager_step", step)
    from transplat_amd import streams

    serial = streams.serial()
    serial.__enter__()
    prof_step()
    torch.cuda.synchronize()
    _lib.prof_enable(info["dominant"])
    n_prof = max(3, min(args.steps, 20))
    for _ in range(n_prof):
        prof_step()
    ms, launches = _lib.prof_read()
    _lib.prof_enable(None)
    if launches == 0 or ms <= 0:
        raise RuntimeError(f"dominant kernel {info['dominant']!r} was not launched in the profiling pass")
    avg_ms = ms / launches
    if info.get("bound", "hbm") == "mfma":
        achieved = info["alg_flops_per_launch"] / (avg_ms * 1e-3) / 1e12
        peak, unit = info.get("peak_tflops", FP32_MFMA_PEAK_TFS), "TFLOP/s"
    else:
        achieved = info["alg_bytes_per_launch"] / (avg_ms * 1e-3) / 1e9
        peak, unit = HBM_PEAK_GBS, "GB/s"

    traffic, traffic_src = committed_traffic(info["dominant"], attn_dtype if info["dominant"] == "win_attn" else "fp32",
                                             args.batch)

    # the step's largest hand-written kernel by time (SURVEY §8d's kernel #1 above stays the
    # headline roofline): the Winograd convolution launches of one step, timed the same way
    conv_roofline = None
    if args.workload == "e2e" and args.dense_dtype in ("fp32", "bf16x3"):
        from transplat_amd import kernels as K

        K.WINO_FLOP_LOG = []
        _lib.prof_enable("wino_conv")
        for _ in range(n_prof):
            prof_step()
        cms, claunches = _lib.prof_read()
        _lib.prof_enable(None)
        log, K.WINO_FLOP_LOG = K.WINO_FLOP_LOG, None
        if claunches and cms > 0 and len(log) == claunches:
            gemm = sum(f for f, _ in log) / (cms * 1e-3) / 1e12
            direct = sum(f for _, f in log) / (cms * 1e-3) / 1e12
            if args.dense_dtype == "bf16x3":
                # three bf16 MFMA products per fp32 product, priced against the dense bf16 peak
                c_achieved, c_peak = 3 * gemm, BF16_MFMA_PEAK_TFS
                flops = ("bf16 MFMA products 3 * 2*16*ci*co*tiles (hi*hi + hi*lo + lo*hi of the 16 F(2x2,3x3) "
                         "GEMMs, unpadded)")
            else:
                c_achieved, c_peak = gemm, FP32_MFMA_PEAK_TFS
                flops = "Winograd GEMM products 2*16*ci*co*tiles (the 16 F(2x2,3x3) GEMMs, unpadded)"
            conv_roofline = {
                "kernel": "wino_conv" if args.dense_dtype == "fp32" else "wino_conv_bf16x3", "bound": "mfma",
                "achieved": c_achieved, "peak": c_peak, "unit": "TFLOP/s", "frac": c_achieved / c_peak,
                "flops": flops,
                "fp32_gemm_equivalent_achieved": gemm, "direct_equivalent_achieved": direct,
                "launches_per_step": claunches / n_prof,
                "ms_per_step": cms / n_prof, "share_of_step": cms / n_prof / (elapsed / args.steps * 1e3),
            }

    # the split-bf16 GEMM launches of one step (DINOv2 / MVT linears, csrc/gemm.hip), timed the same way
    gemm_roofline = None
    if args.workload == "e2e" and args.dense_dtype == "bf16x3":
        from transplat_amd import kernels as K

        K.GEMM_LOG = []
        _lib.prof_enable("gemm_x3")
        for _ in range(n_prof):
            prof_step()
        gms, glaunches = _lib.prof_read()
        _lib.prof_enable(None)
        glog, K.GEMM_LOG = K.GEMM_LOG, None
        if glaunches and gms > 0 and len(glog) == glaunches:
            flops = sum(3 * 2 * m * n * k for m, n, k, _ in glog)
            g_achieved = flops / (gms * 1e-3) / 1e12
            gemm_roofline = {
                "kernel": "gemm_x3", "bound": "mfma", "achieved": g_achieved, "peak": BF16_MFMA_PEAK_TFS,
                "unit": "TFLOP/s", "frac": g_achieved / BF16_MFMA_PEAK_TFS,
                "flops": "bf16 MFMA products 3 * 2*m*n*k per launch (hi*hi + hi*lo + lo*hi)",
                "launches_per_step": glaunches / n_prof, "ms_per_step": gms / n_prof,
                "share_of_step": gms / n_prof / (elapsed / args.steps * 1e3),
            }

    render_valu = render_valu_roofline(step, n_prof) if args.workload == "raster" else None
    serial.__exit__(None, None, None)
    result = {
        "roofline": {
            "kernel": info["dominant"],
            "bound": info.get("bound", "hbm"),
            "achieved": achieved,
            "peak": peak,
            "unit": unit,
            "frac": achieved / peak,
            "traffic": traffic,
            "traffic_unit": "bytes/launch (HBM, PMC FETCH_SIZE x2 + WRITE_SIZE)",
            "traffic_source": traffic_src,
            "avg_launch_ms": avg_ms,
            "launches": launches,
        },
    }
    if "fp32_equivalent_flops_per_launch" in info:
        result["roofline"]["flops_note"] = info["flops_note"]
        result["roofline"]["fp32_equivalent_achieved"] = info["fp32_equivalent_flops_per_launch"] / (avg_ms * 1e-3) / 1e12
    if conv_roofline is not None:
        result["roofline_step_dominant"] = conv_roofline
    if gemm_roofline is not None:
        result["roofline_gemm"] = gemm_roofline
    if render_valu is not None:
        result["roofline_render_valu"] = render_valu
    return result


if __name__ == "__main__":
    main()
