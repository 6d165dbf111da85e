#!/usr/bin/env python
"""bench.py -- images/sec of the SDXL-base sampling hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one batch of synthetic input per GPU: ONE 1024x1024 image =
`Diffuser::sample_latent` with n_steps=30 (which the reference executes as 31 CFG UNet step pairs, stablediffusion/mod.rs:
400-406) at CFG 7.5, followed by `LatentDecoder::latent_to_image` -- BASELINE.json configs[1] (429.7 TFLOP/image, SURVEY
section 8d).  Inputs (conditioning, noise) are synthetic seeded tensors already resident in HBM when the timed region
starts; weights are the seeded synthetic SDXL-base architecture (no checkpoint can be downloaded here).  With N>1 every
rank renders its own prompt (weak scaling, no collective in the loop) after ONE RCCL broadcast of the packed weight arena
from rank 0 over xGMI; value = total images of all ranks / max-over-ranks wall time.

A plain run sets up, warms up, times --steps images and prints the JSON line (value, ms_per_step, unet_step_ms_p50, ...).
--dump-outputs DIR also writes what the last timed image returned to its caller (the latent, the u8 image as float32) as
DIR/<name>.npy, for comparing two builds output for output.  --full adds the measurements below, each of which takes runs
of its own; without it their objects are null on the line.

Extra objects on the JSON line (--full):
  decode_ms     latent_to_image timed on its own, 3 calls after the timed region.
  roofline      live hipEvent measurement of the dominant kernel (the implicit-GEMM conv/linear kernel, which carries
                ~94% of the algorithmic FLOPs): achieved = sum of its algorithmic FLOPs (2*M*N*K per launch, unpadded) /
                sum of its launch durations over one UNet forward of the timed configuration; peak = 2500 TFLOP/s
                (dense fp16 MFMA, MI355X_MICROARCH.md).
  cpu_baseline  the oracle (torch-CPU fp32 restatement of the reference graph; the reference's burn-ndarray path cannot
                be built here) timed on this box's host cores on a bounded sample, rank 0 / N=1 only.
  parity        the committed parity report under profiles/ and, for config 2 at 1024^2 on one GPU, parity measured in
                this run against tests/golden/ fixtures; strict_f32 = the fp32-class engines timed on the same trajectory.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

TFLOP_PER_UNET_FWD_1024 = 6.761      # SURVEY section 8(d), base UNet, latent 128x128, B=1
TFLOP_VAE_DECODE_1024 = 10.470
TFLOP_PER_UNET_FWD_512 = 1.589
TFLOP_VAE_DECODE_512 = 2.515
PEAK_F16_TFLOPS = 2500.0             # dense fp16 MFMA peak, MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3


# ------------------------------------------------------------------------------------------ distributed helpers
def dist_env():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def init_dist(backend: str):
    import torch.distributed as dist
    rank, local_rank, world = dist_env()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_rank, world


def broadcast_arena(arena_u8, src: int = 0, chunk_bytes: int = 1 << 30):
    """fallback one-time weight broadcast through torch.distributed (RCCL on GPUs, gloo in the CPU tests), in <=1 GiB
    pieces -- used when the library's own communicator (make_comm / Comm.bcast_*) cannot be created"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    n = arena_u8.numel()
    for o in range(0, n, chunk_bytes):
        dist.broadcast(arena_u8[o:min(n, o + chunk_bytes)], src=src)


def scatter_allgather_arena(arena_u8, plan_fn, src: int = 0):
    """the LIBRARY's broadcast schedule (csrc/comm.cpp: scatter of `world` equal pieces from the root, in-place all-gather,
    small tail broadcast) executed over torch.distributed point-to-point / collective calls.  plan_fn(nbytes, world, rank)
    is the library's sdxl_bcast_plan.  The engine runs the same plan over RCCL inside sdxl_*_bcast_weights; this host-side
    twin exists so that world-size-2 gloo tests push a real weight-arena byte image through the same offsets."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    rank, world, n = dist.get_rank(), dist.get_world_size(), arena_u8.numel()
    poff, plen, toff, tlen = plan_fn(n, world, rank)
    if plen > 0:
        if rank == src:
            reqs = [dist.isend(arena_u8[plan_fn(n, world, r)[0]:plan_fn(n, world, r)[0] + plen], dst=r) for r in range(world) if r != src]
            for q in reqs:
                q.wait()
        else:
            dist.recv(arena_u8[poff:poff + plen], src=src)
        pieces = [torch.empty(plen, dtype=arena_u8.dtype, device=arena_u8.device) for _ in range(world)]
        dist.all_gather(pieces, arena_u8[poff:poff + plen].clone())
        for r in range(world):
            o = plan_fn(n, world, r)[0]
            arena_u8[o:o + plen] = pieces[r]
    if tlen > 0:
        dist.broadcast(arena_u8[toff:toff + tlen], src=src)


def make_comm(pkg, local_rank: int):
    """the engine's own RCCL communicator: rank 0 draws the unique id, the existing torch.distributed group ships it"""
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()
    box = [pkg.Comm.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    return pkg.Comm(local_rank, rank, world, box[0])


def max_over_ranks(seconds: float, device) -> float:
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return seconds
    t = torch.tensor([seconds], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(x: float, device) -> float:
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def barrier():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


def prompt_seed(rank: int, step: int) -> int:
    """prompt i -> GPU i mod N: every (rank, step) pair is an independent synthetic prompt"""
    return 1000 + 97 * rank + step


DUMP_BUDGET_BYTES = 60 << 20         # --dump-outputs: all arrays together stay under 64 MB


def dump_outputs(out_dir: str, arrays: dict, budget: int = DUMP_BUDGET_BYTES) -> None:
    """writes each tensor as out_dir/<name>.npy in float32.  When together they exceed `budget`, each is replaced by the same
    share of its flattened elements, drawn once with a fixed seed (identical indices on every run with the same arguments)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = 4 * sum(t.numel() for t in arrays.values())
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if total > budget:
            k = max(1, a.size * budget // total)
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, size=k, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------ CPU baseline
def effective_cores() -> int:
    """cores this process may really use: min(affinity mask, cgroup cpu quota) -- os.cpu_count() reports the host's
    256 hardware threads inside a quota-limited container, and 256 OpenMP threads on a handful of cores thrash."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as fh:
                txt = fh.read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                        n = min(n, max(1, int(q / int(fh.read()) + 0.5)))
        except Exception:
            pass
    return max(1, n)


def cpu_baseline(res: int, budget_s: float = 30.0):
    """The oracle (fp32 torch-CPU restatement of the reference graph) timed on the host cores on a BOUNDED sample of the same
    workload: ONE full `UNet::forward` of the SDXL-base architecture at the benchmarked resolution (B=1, as the reference runs
    it: 6.761 TFLOP at 1024x1024, ~20-40 s on 8-16 cores) -- the unit the 31 x 2 forwards of one image repeat; images/sec
    follows by FLOPs (the VAE decode, 2.4 % of the job, is credited at the same rate).  Weights are random tensors of the real
    shapes (a pool copied into per-parameter storage: the oracle's seeded numpy recipe takes ~100 s for 2.6 G values and
    timing does not depend on the values)."""
    import torch
    from oracle import config as OC, model as OM
    cores = effective_cores()
    threads = min(cores, 32)
    torch.set_num_threads(threads)
    cfg = OC.sdxl_base_config()
    t0 = time.time()
    specs = OC.unet_param_specs(cfg)
    pool = (torch.rand(max(p.numel for p in specs), generator=torch.Generator().manual_seed(0)) - 0.5)
    W = {}
    for p in specs:
        W[p.name] = (pool[:p.numel] * float(p.scale) + float(p.mean)).reshape(p.shape)
    t_w = time.time() - t0
    lat = res // 8
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 4, lat, lat, generator=g)
    ctx = torch.randn(1, 77, cfg.context_dim, generator=g)
    y = torch.randn(1, cfg.adm_in_channels, generator=g)
    fwd_tf = {1024: TFLOP_PER_UNET_FWD_1024, 512: TFLOP_PER_UNET_FWD_512}.get(res, TFLOP_PER_UNET_FWD_1024 * (res / 1024.0) ** 2)
    with torch.no_grad():
        t0 = time.time()
        out = OM.unet_forward(cfg, W, x, torch.tensor([500]), ctx, y)
        dt_ = time.time() - t0
    print(f"[cpu_baseline] oracle UNet::forward {res}x{res}: {dt_:.1f} s on {threads} threads (weights {t_w:.1f} s, not timed)", file=sys.stderr, flush=True)
    tf_per_s = fwd_tf / dt_
    scale = (res / 1024.0) ** 2
    tflop_image = (62 * TFLOP_PER_UNET_FWD_1024 + TFLOP_VAE_DECODE_1024) * scale
    return {"value": tf_per_s / tflop_image, "unit": "images/sec", "cores": threads, "kind": "port",
            "method": "oracle, one UNet forward timed end to end, images/sec extrapolated by FLOPs",
            "sample": (f"ONE full oracle UNet::forward at {res}x{res} (B=1, {fwd_tf:.3f} TFLOP) timed end to end: {dt_:.1f} s = {tf_per_s:.3f} TFLOP/s on "
                       f"{threads} threads (host reports {os.cpu_count()} cpus, {cores} usable; output finite: {bool(torch.isfinite(out).all())}); "
                       f"images/sec = that rate over the {tflop_image:.1f} TFLOP of one image (31 CFG step pairs = 62 forwards + VAE decode)"),
            "tflops": tf_per_s}


# ------------------------------------------------------------------------------------------ oracle end to end (config 1)
def cpu_oracle_config1():
    """BASELINE configs[0] on the host cores, END TO END: the oracle's Diffuser::sample_latent (SDXL-base, 512x512, 4 steps,
    CFG 1.0 -> 8 UNet forwards) + LatentDecoder::latent_to_image, same seeds as tests/golden/fullsize_config1.npz
    (15.2 TFLOP; ~0.5-1.5 minutes on 8-16 cores).  The reported proxy for the reference's burn-ndarray path."""
    import numpy as np
    import torch
    from oracle import config as OC, make_golden_fullsize as MG, pipeline as OP
    cores = effective_cores()
    threads = min(cores, 32)
    torch.set_num_threads(threads)
    t0 = time.time()
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):      # (the fixture generator narrates on stdout; the bench prints ONE JSON line there)
        cfg, W = MG.base_weights()
        v, Wv = MG.vae_weights()
    t_w = time.time() - t0
    i = MG.config1_inputs(cfg)
    cond = OP.Conditioning(i["uctx"], None, i["ctx"], None, i["uy"], None, i["y"], None, (512, 512))
    with torch.no_grad():
        t0 = time.time()
        lat = OP.Diffuser(cfg, W, OC.alphas_cumprod()).sample_latent(cond, 1.0, 4, i["noise"])
        t1 = time.time()
        OP.LatentDecoder(v, Wv).latent_to_image(lat)
        t2 = time.time()
    gold = os.path.join(ROOT, "tests", "golden", "fullsize_config1.npz")
    dev = None
    if os.path.exists(gold):
        ref = torch.from_numpy(np.load(gold)["latent"])
        dev = float((lat - ref).abs().max() / ref.abs().max())
    total = t2 - t0
    tflop = 8 * TFLOP_PER_UNET_FWD_512 + TFLOP_VAE_DECODE_512
    return {"value": 1.0 / total, "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": (f"the WHOLE config-1 job on the host: oracle sample_latent (8 UNet forwards at 512x512) {t1 - t0:.1f} s + "
                       f"latent_to_image {t2 - t1:.1f} s = {total:.1f} s on {threads} threads (host reports {os.cpu_count()} cpus, "
                       f"{cores} usable); synthetic fp32 weights generated in {t_w:.0f} s (not timed); "
                       f"latent vs the committed oracle fixture: rel {dev if dev is None else format(dev, '.2e')}"),
            "tflops": tflop / total, "seconds": {"sample_latent": t1 - t0, "latent_to_image": t2 - t1}}, lat


def load_parity():
    """parity evidence measured by tests/test_gpu_baseline_parity.py on an MI355X (committed summaries under profiles/): the
    STATIC part of the line's parity object -- what live_parity() below does not re-measure in this run"""
    out = {}
    try:
        name = next(n for n in ("r06_parity_baseline.json", "r05_parity_baseline.json", "r04_parity_baseline.json", "r03_parity_baseline.json", "r02_parity_baseline.json") if os.path.exists(os.path.join(ROOT, "profiles", n)))
        with open(os.path.join(ROOT, "profiles", name)) as fh:
            r = json.load(fh)
        c1 = r.get("config1_f32_vs_oracle", {}).get("final")
        if c1:
            out["config1_f32_vs_oracle_latent_max_abs"] = c1["max_abs"]
            out["config1_f32_vs_oracle_latent_rel"] = c1["rel"]
        u = r.get("unet_forward_1024_vs_oracle", {})
        for k in ("f32", "f32_split", "f32_split_mix", "f16", "f16_f32res"):
            if k in u:
                out[f"unet_forward_1024_{k}_vs_oracle_rel"] = u[k]["rel"]
        if "reference_f16_class" in u:      # the oracle in the reference's own GPU arithmetic (LibTorch<f16>: every op output an f16 tensor) vs the fp32 oracle
            out["unet_forward_1024_reference_f16_class_rel"] = u["reference_f16_class"]["rel"]
            out["unet_forward_1024_oracle_f16_operand_model_rel"] = u.get("oracle_f16_operand_model_rel")
        t = r.get("config2_trajectory", {})
        if "f32_vs_oracle" in t:
            out["config2_f32_vs_oracle_final_max_abs"] = t["f32_vs_oracle"]["final"]["max_abs"]
            out["config2_f32_vs_oracle_final_rel"] = t["f32_vs_oracle"]["final"]["rel"]
        if "reference_f16_class" in t:    # the oracle's own 31-step trajectory in the reference's f16 arithmetic (LibTorch<f16>) vs its fp32 trajectory
            out["config2_reference_f16_class_final_max_abs"] = t["reference_f16_class"]["final"]["max_abs"]
            out["config2_reference_f16_class_final_rel"] = t["reference_f16_class"]["final"]["rel"]
        for k in ("f32_split_mix", "f16", "f16_f32res"):
            if k + "_vs_oracle" in t:
                out[f"config2_{k}_vs_oracle_final_max_abs"] = t[k + "_vs_oracle"]["final"]["max_abs"]
        for k in ("f16", "f16_f32res"):
            if k + "_vs_f32" in t:
                out[f"config2_{k}_vs_f32_final_rel"] = t[k + "_vs_f32"][-1]["rel"]
                out[f"config2_{k}_vs_f32_final_max_abs"] = t[k + "_vs_f32"][-1]["max_abs"]
        d = r.get("decode_1024_vs_oracle", {})
        for k in ("f32", "f32_split", "f16"):
            if k in d:
                out[f"decode_1024_{k}_vs_oracle_image_max_abs"] = d[k]["image_sub"]["max_abs"]
                out[f"decode_1024_{k}_u8_max_diff"] = d[k]["u8_max_diff"]
        for key, tag in (("refiner_forward_1024_vs_oracle", "refiner_forward_1024"), ("unet_forward_1024_f16_weights_vs_oracle", "unet_forward_1024_f16_weights")):
            for k, v in r.get(key, {}).items():
                out[f"{tag}_{k}_vs_oracle_rel"] = v["rel"]
        for key, tag in (("refine_latent_1024_vs_oracle", "refine_latent_1024"), ("inpainting_1024_vs_oracle", "inpainting_1024")):
            for k, v in r.get(key, {}).items():
                out[f"{tag}_{k}_vs_oracle_final_max_abs"] = v["final"]["max_abs"]
                out[f"{tag}_{k}_vs_oracle_final_rel"] = v["final"]["rel"]
        for k, v in r.get("encode_1024_vs_oracle", {}).items():
            out[f"encode_1024_{k}_vs_oracle_rel"] = v["rel"]
        out["source"] = f"profiles/{name} (tests/test_gpu_baseline_parity.py on MI355X; committed, NOT measured in this run)"
        out["latent_tolerance"] = ("north_star's 1e-3 on latents (unscaled) is met by SDXL_DTYPE_F32 and SDXL_DTYPE_F32_SPLIT; SDXL_DTYPE_F32_SPLIT_MIX is inside the tests' scaled bound "
                                   "at config 2 only; the f16 mode reports its measured drift, 4.9x inside the reference's own f16 numerical class")
    except Exception:
        return None
    return out


def _seeded(*shape, seed):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rel(out, ref):
    d = (out.detach().float().cpu() - ref).abs().max()
    return float(d), float(d / ref.abs().max().clamp_min(1e-30))


def live_parity(pkg, ctx, diffuser, decoder, prec: str, vae_prec: str, weights: str = "fp32"):
    """Parity MEASURED IN THIS RUN (rank 0, after the timed region) against the committed oracle fixtures tests/golden/fullsize_*.npz
    (oracle/make_golden_fullsize.py; only the fixture files are read -- nothing under oracle/ executes here):
      * one base UNet::forward at 1024x1024 on the timed engine;
      * one latent_to_image at 1024x1024 on the timed VAE;
      * BASELINE configs[1] itself -- 1024x1024, 31 CFG-7.5 iterations -- on the fixture's inputs: the timed engine's final latent
        and the strict-fp32 engine's (SDXL_DTYPE_F32, exact-fp32 MFMA), the latter TIMED: `strict_f32` = the throughput of the
        mode that meets north_star's 1e-3, next to the benchmarked one."""
    import numpy as np
    import torch
    gold = os.path.join(ROOT, "tests", "golden")
    cfg = pkg.sdxl_base_config()
    out, strict = {}, None
    wsuf = "_f16w" if weights == "f16" else ""          # the timed engine's own fixtures: the oracle on the SAME (f16-representable) weights
    g = np.load(os.path.join(gold, f"fullsize_unet1024{wsuf}.npz"))
    x, t = _seeded(1, 4, 128, 128, seed=111), torch.tensor([500], dtype=torch.int32)
    c, y = _seeded(1, 77, cfg.context_dim, seed=112), _seeded(1, cfg.adm_in_channels, seed=113)
    o = diffuser.diffusion.forward(x.cuda(), t.cuda(), c.cuda(), y.cuda())
    out[f"unet_forward_1024_{prec}_vs_oracle_rel"] = _rel(o, torch.from_numpy(g["out"]))[1]
    gdec = os.path.join(gold, f"fullsize_decode1024{wsuf}.npz")
    g = np.load(gdec if os.path.exists(gdec) else os.path.join(gold, "fullsize_decode1024.npz"))
    out["decode_fixture"] = os.path.basename(gdec) if os.path.exists(gdec) else "fullsize_decode1024.npz (fp32 weights: the f16-weights decode fixture is missing)"
    latent = _seeded(1, 4, 128, 128, seed=121).cuda()
    img = decoder.decode_latent(latent).cpu()
    out[f"decode_1024_{vae_prec}_vs_oracle_image_max_abs"] = _rel(img[:, :, ::5, ::5], torch.from_numpy(g["image_sub"]))[0]
    u8 = decoder.latent_to_image(latent).buffer.cpu().numpy()
    d8 = np.abs(u8[:, ::5, ::5].astype(np.int32) - g["u8_sub"].astype(np.int32))
    out[f"decode_1024_{vae_prec}_u8_max_diff"] = int(d8.max())
    out[f"decode_1024_{vae_prec}_u8_frac_diff"] = float((d8 > 0).mean())
    gp = os.path.join(gold, "fullsize_config2.npz")
    if os.path.exists(gp):
        g = np.load(gp)
        ref = torch.from_numpy(g["latent"])
        ref_timed = torch.from_numpy(np.load(os.path.join(gold, f"fullsize_config2{wsuf}.npz"))["latent"])
        i = dict(noise=_seeded(1, 4, 128, 128, seed=131), ctx=_seeded(1, 77, cfg.context_dim, seed=132), uctx=_seeded(77, cfg.context_dim, seed=133),
                 y=_seeded(1, cfg.adm_in_channels, seed=134), uy=_seeded(cfg.adm_in_channels, seed=135))
        cond = pkg.Conditioning(context_full=i["ctx"].cuda(), channel_context=i["y"].cuda(), unconditional_context_full=i["uctx"].cuda(),
                                unconditional_channel_context=i["uy"].cuda(), resolution=(1024, 1024))
        lat = diffuser.sample_latent(cond, 7.5, 30, i["noise"].cuda())
        a, r = _rel(lat, ref_timed)
        out[f"config2_{prec}{wsuf}_vs_oracle_final_max_abs"], out[f"config2_{prec}{wsuf}_vs_oracle_final_rel"] = a, r
        strict = {}
        lat_bound = 1e-3 * max(1.0, float(ref.abs().max()) / 4.0)     # the parity tests' bar: north_star's 1e-3 at SDXL's latent scale (|x| <~ 4), scaled with the synthetic trajectory
        out["timed_engine"] = {"precision": prec, "weights": weights, "config2_final_latent_max_abs_vs_oracle": a, "meets_1e-3": bool(a <= 1e-3),
                               "lat_bound_scaled": 1e-3 * max(1.0, float(ref_timed.abs().max()) / 4.0),
                               "inside_lat_bound_scaled": bool(a <= 1e-3 * max(1.0, float(ref_timed.abs().max()) / 4.0))}
        for tag, dtv, what in (("f32", pkg.DTYPE_F32, "SDXL_DTYPE_F32 UNet (exact-fp32 MFMA) + the timed VAE"),
                               ("f32_split", pkg.DTYPE_F32_SPLIT, "SDXL_DTYPE_F32_SPLIT UNet (fp32 stream, (hi, lo) f16 operands x 3 MFMAs in the GEMMs and in the attention) + the timed VAE"),
                               ("f32_split_mix", pkg.DTYPE_F32_SPLIT_MIX, "SDXL_DTYPE_F32_SPLIT_MIX UNet (the split engine with the self-attention and the GEGLU projection on plain f16 "
                                "operands -- the two classes the measured precision frontier affords, profiles/r05_precision_frontier.json) + the timed VAE")):
            if prec == tag and weights == "fp32":
                continue
            d32 = pkg.Diffuser(ctx, cfg, dtv, seed=0)
            d32.enable_step_timing(True)
            d32.sample_latent(cond, 7.5, 2, i["noise"].cuda())            # plan + hipGraph capture (3 iterations)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lat32 = d32.sample_latent(cond, 7.5, 30, i["noise"].cuda())
            steps = d32.step_times_ms()
            decoder.latent_to_image(lat32)
            torch.cuda.synchronize()
            dt_ = time.perf_counter() - t0
            a, r = _rel(lat32, ref)
            out[f"config2_{tag}_vs_oracle_final_max_abs"], out[f"config2_{tag}_vs_oracle_final_rel"] = a, r
            strict[tag] = {"precision": what, "images_per_sec": round(1.0 / dt_, 4),
                           "unet_step_ms": round(statistics.median(steps), 2) if steps else None, "images_timed": 1,
                           "config2_final_latent_max_abs_vs_oracle": a, "meets_1e-3": bool(a <= 1e-3),
                           "lat_bound_scaled": lat_bound, "inside_lat_bound_scaled": bool(a <= lat_bound)}
            del d32
        # the same split-operand engine on the weights a real SDXL record holds (every parameter an f16 value, sample/main.rs:37): the packed
        # lo halves are zero and the GEMMs leave out the w_lo x a_hi MFMAs; parity against the oracle's own trajectory ON THOSE WEIGHTS
        gpw = os.path.join(gold, "fullsize_config2_f16w.npz")
        if os.path.exists(gpw) and hasattr(pkg, "SEED_F16_WEIGHTS"):
            refw = torch.from_numpy(np.load(gpw)["latent"])
            dw = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F32_SPLIT, seed=pkg.SEED_F16_WEIGHTS)
            dw.enable_step_timing(True)
            dw.sample_latent(cond, 7.5, 2, i["noise"].cuda())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            latw = dw.sample_latent(cond, 7.5, 30, i["noise"].cuda())
            steps = dw.step_times_ms()
            decoder.latent_to_image(latw)
            torch.cuda.synchronize()
            dt_ = time.perf_counter() - t0
            a, r = _rel(latw, refw)
            out["config2_f16weights_f32_split_vs_oracle_final_max_abs"], out["config2_f16weights_f32_split_vs_oracle_final_rel"] = a, r
            dm = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F32_SPLIT_MIX, seed=pkg.SEED_F16_WEIGHTS)
            dm.enable_step_timing(True)
            dm.sample_latent(cond, 7.5, 2, i["noise"].cuda())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            latm = dm.sample_latent(cond, 7.5, 30, i["noise"].cuda())
            stepsm = dm.step_times_ms()
            decoder.latent_to_image(latm)
            torch.cuda.synchronize()
            dtm = time.perf_counter() - t0
            am, rm = _rel(latm, refw)
            out["config2_f16weights_f32_split_mix_vs_oracle_final_max_abs"], out["config2_f16weights_f32_split_mix_vs_oracle_final_rel"] = am, rm
            lbw = 1e-3 * max(1.0, float(refw.abs().max()) / 4.0)
            strict["f32_split_mix_f16_weights"] = {
                "precision": "SDXL_DTYPE_F32_SPLIT_MIX UNet on f16-representable weights (what the reference's records hold) + the timed VAE; oracle = the same weights",
                "images_per_sec": round(1.0 / dtm, 4), "unet_step_ms": round(statistics.median(stepsm), 2) if stepsm else None, "images_timed": 1,
                "config2_final_latent_max_abs_vs_oracle": am, "meets_1e-3": bool(am <= 1e-3), "lat_bound_scaled": lbw, "inside_lat_bound_scaled": bool(am <= lbw)}
            del dm
            d5 = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F32_SPLIT_MIX_F16W, seed=pkg.SEED_F16_WEIGHTS)
            d5.enable_step_timing(True)
            d5.sample_latent(cond, 7.5, 2, i["noise"].cuda())
            torch.cuda.synchronize()
            N5 = 3                 # images timed (sampling + decode each, same prompt: the arithmetic does not depend on the data)
            steps5 = []
            t0 = time.perf_counter()
            for _ in range(N5):
                lat5 = d5.sample_latent(cond, 7.5, 30, i["noise"].cuda())
                steps5 += d5.step_times_ms()
                decoder.latent_to_image(lat5)
            torch.cuda.synchronize()
            dt5 = (time.perf_counter() - t0) / N5
            a5, r5 = _rel(lat5, refw)
            out["config2_f16weights_f32_split_mix_f16w_vs_oracle_final_max_abs"], out["config2_f16weights_f32_split_mix_f16w_vs_oracle_final_rel"] = a5, r5
            strict["f32_split_mix_f16w_mode_f16_weights"] = {
                "precision": "SDXL_DTYPE_F32_SPLIT_MIX_F16W UNet (split engine; self-attention, both attentions' out-projections, GEGLU, QKV projection, FF-out and the cross-attention query "
                             "projection on plain f16 operands, LayerNorms folded through the f16 shadow of the stream: the classes the measured frontier affords when the parameters are exact f16 "
                             "values) on f16-representable weights + the timed VAE; oracle = the same weights",
                "mix_classes": d5.diffusion.mix_classes(),
                "images_per_sec": round(1.0 / dt5, 4), "unet_step_ms": round(statistics.median(steps5), 2) if steps5 else None, "images_timed": N5,
                "config2_final_latent_max_abs_vs_oracle": a5, "meets_1e-3": bool(a5 <= 1e-3), "lat_bound_scaled": lbw, "inside_lat_bound_scaled": bool(a5 <= lbw),
                "meets_1_img_per_sec_inside_scaled_bound": bool(a5 <= lbw and 1.0 / dt5 >= 1.0)}
            del d5
            if hasattr(pkg, "DTYPE_F32_SPLIT_MIX_F16W_GEGLU2"):
                d6 = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F32_SPLIT_MIX_F16W_GEGLU2, seed=pkg.SEED_F16_WEIGHTS)
                d6.enable_step_timing(True)
                d6.sample_latent(cond, 7.5, 2, i["noise"].cuda())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lat6 = d6.sample_latent(cond, 7.5, 30, i["noise"].cuda())
                steps6 = d6.step_times_ms()
                decoder.latent_to_image(lat6)
                torch.cuda.synchronize()
                dt6 = time.perf_counter() - t0
                a6, r6 = _rel(lat6, refw)
                out["config2_f16weights_f32_split_mix_f16w_geglu2_vs_oracle_final_max_abs"] = a6
                strict["f32_split_mix_f16w_geglu2_mode_f16_weights"] = {
                    "precision": "SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2 UNet (F16W with the GEGLU projection's activations as (hi, lo) f16 pairs along a doubled K: the mode that is inside "
                                 "the scaled bound on every fixture of the parity tests, the 4-step inpainting stress fixture included) on f16-representable weights + the timed VAE",
                    "mix_classes": d6.diffusion.mix_classes(),
                    "images_per_sec": round(1.0 / dt6, 4), "unet_step_ms": round(statistics.median(steps6), 2) if steps6 else None, "images_timed": 1,
                    "config2_final_latent_max_abs_vs_oracle": a6, "meets_1e-3": bool(a6 <= 1e-3), "lat_bound_scaled": lbw, "inside_lat_bound_scaled": bool(a6 <= lbw)}
                del d6
            if hasattr(pkg, "DTYPE_F32_SPLIT_F16W"):
                d7 = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F32_SPLIT_F16W, seed=pkg.SEED_F16_WEIGHTS)
                d7.enable_step_timing(True)
                d7.sample_latent(cond, 7.5, 2, i["noise"].cuda())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lat7 = d7.sample_latent(cond, 7.5, 30, i["noise"].cuda())
                steps7 = d7.step_times_ms()
                decoder.latent_to_image(lat7)
                torch.cuda.synchronize()
                dt7 = time.perf_counter() - t0
                a7, r7 = _rel(lat7, refw)
                out["config2_f16weights_f32_split_f16w_vs_oracle_final_max_abs"] = a7
                strict["f32_split_f16w_mode_f16_weights"] = {
                    "precision": "SDXL_DTYPE_F32_SPLIT_F16W UNet (F32_SPLIT's fp32-class arithmetic with the transformer's linear layers on the f16 kernels: HL16 rows read as f16 rows of twice the width, "
                                 "weights packed twice per 16-channel group; split-precision cross-attention inside the query projection) on f16-representable weights + the timed VAE",
                    "mix_classes": d7.diffusion.mix_classes(),
                    "images_per_sec": round(1.0 / dt7, 4), "unet_step_ms": round(statistics.median(steps7), 2) if steps7 else None, "images_timed": 1,
                    "config2_final_latent_max_abs_vs_oracle": a7, "meets_1e-3": bool(a7 <= 1e-3)}
                del d7
            strict["f32_split_f16_weights"] = {
                "precision": "SDXL_DTYPE_F32_SPLIT UNet on f16-representable weights (what the reference's records hold): two MFMAs per GEMM product, "
                             "three in the attention + the timed VAE; oracle = the same weights, tests/golden/fullsize_config2_f16w.npz",
                "images_per_sec": round(1.0 / dt_, 4), "unet_step_ms": round(statistics.median(steps), 2) if steps else None, "images_timed": 1,
                "config2_final_latent_max_abs_vs_oracle": a, "meets_1e-3": bool(a <= 1e-3)}
            del dw
        strict = strict or None
    out["source"] = "measured in this run against tests/golden/fullsize_{unet1024,decode1024,config2}.npz (committed oracle outputs)"
    return out, strict


# ------------------------------------------------------------------------------------------ main
CONFIGS = {
    1: dict(res=512, n_steps=4, cfg=1.0, label="BASELINE configs[0]: SDXL-base 512x512, n_steps=4 (4 CFG pairs, both branches evaluated), CFG 1.0 + VAE decode to u8"),
    2: dict(res=1024, n_steps=30, cfg=7.5, label="BASELINE configs[1]"),
    4: dict(res=1024, n_steps=50, cfg=7.5, label="BASELINE configs[3]: SDXL-base 50 CFG pairs + refiner refine_latent(step_start=800, n_steps=50 -> 10 single forwards) + VAE decode to u8"),
    5: dict(res=1024, n_steps=100, cfg=7.5, label="BASELINE configs[4]: inpainting -- u8 reference -> VAE encode, 100 CFG pairs with the per-step blend (mask = latent rows 0..25 generated), VAE decode to u8"),
}
TFLOP_REFINER_FWD_1024 = 7.286


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed images per GPU")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: decode_ms, roofline, cpu_baseline, parity / strict_f32 "
                         "(off: those objects are null on the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed image's outputs (latent, u8 image) as DIR/<name>.npy in float32")
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS), help="BASELINE.json configs index + 1 (2 = the metric's)")
    ap.add_argument("--res", type=int, default=None)
    ap.add_argument("--n-steps", type=int, default=None, help="--n-diffusion-steps of the reference CLI (30 -> 31 iterations)")
    ap.add_argument("--cfg", type=float, default=None)
    ap.add_argument("--dtype", default="f16", choices=["f16", "f32", "f16_f32res", "f32_split", "f32_split_mix", "f32_split_mix_f16w", "f32_split_mix_f16w_geglu2", "f32_split_f16w"],
                    help="UNet arithmetic: f16 (the reference's GPU precision, src/bin/sample/main.rs:122), f16_f32res, f32 (exact-fp32 MFMA: the strict-parity "
                         "mode), f32_split (fp32-class: fp32 stream, (hi, lo) f16 operands with three MFMAs per product in the GEMMs and in the attention), "
                         "f32_split_mix (+ self-attention and GEGLU on plain f16) or f32_split_mix_f16w (+ six more transformer classes on plain f16: for "
                         "f16-representable parameters, i.e. with --weights f16; on other weights the engine falls back to f32_split_mix's classes)")
    ap.add_argument("--weights", default="fp32", choices=["fp32", "f16"],
                    help="synthetic UNet parameters as drawn (fp32) or rounded to IEEE f16 first -- what the reference's records hold "
                         "(HalfPrecisionSettings, src/bin/sample/main.rs:37)")
    ap.add_argument("--vae-dtype", default="f32_split", choices=["f16", "f32", "f32_split"],
                    help="arithmetic of the VAE legs; the reference decodes in f32 (src/bin/sample/main.rs:121,271-278): f32 = exact-fp32 "
                         "MFMA, f32_split = fp32-class results from three f16 MFMAs per product on (hi, lo) operand pairs")
    ap.add_argument("--pipeline-decode", action="store_true",
                    help="decode image i on a second HIP stream under the sampling of image i+1 (measured +0.3 %% only: both legs "
                         "are chip-filling MFMA work; off by default)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out cpu_baseline")
    ap.add_argument("--no-live-parity", action="store_true",
                    help="with --full: skip the parity block measured in this run (config 2 only: 1024^2 forward / decode / the 31-step "
                         "trajectory on the fixture inputs, and the strict-fp32 engine timed on it, ~10 s)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--prompts-per-call", type=int, default=1, choices=[1, 2, 4],
                    help="serving-shape extra (config 2 only): n independent prompts per sample_latent call = UNet batch 2n; "
                         "the default 1 is BASELINE.json's batch-1 configuration")
    ap.add_argument("--unfused-xattn", action="store_true",
                    help="A/B: run the cross-attention as projection + attention kernel instead of inside the projection's epilogue")
    ap.add_argument("--split-cfg", action="store_true",
                    help="run the CFG pair as two concurrent batch-1 chains (measured -2.6 %% step time; off by default so "
                         "the timed launches are the ones the roofline object and the rocprofv3 summary describe)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    C = CONFIGS[args.config]
    res = args.res or C["res"]
    n_steps = args.n_steps or C["n_steps"]
    cfg_scale = C["cfg"] if args.cfg is None else args.cfg

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the engine has no CPU path")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: never answer an N-rank request with a 1-rank line -- start the N ranks
        # ourselves (one process per GPU, rendezvous on 127.0.0.1) exactly as the driver's torch.distributed.run line would
        import socket
        import subprocess
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible on this node")
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    for kv in filter(None, os.environ.get("SDXL_DEBUG_SET", "").split(",")):   # A/B knobs (sdxl_debug_set), e.g. igemm_epilogue_staged=1
        k_, v_ = kv.split("=")
        pkg.debug_set(k_, int(v_))
    rank, local_rank, world = init_dist("nccl")
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}")
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    dts = {"f16": pkg.DTYPE_F16, "f32": pkg.DTYPE_F32, "f16_f32res": pkg.DTYPE_F16_F32RES, "f32_split": pkg.DTYPE_F32_SPLIT,
           "f32_split_mix": pkg.DTYPE_F32_SPLIT_MIX, "f32_split_mix_f16w": pkg.DTYPE_F32_SPLIT_MIX_F16W,
           "f32_split_mix_f16w_geglu2": pkg.DTYPE_F32_SPLIT_MIX_F16W_GEGLU2, "f32_split_f16w": pkg.DTYPE_F32_SPLIT_F16W}
    dt, vdt = dts[args.dtype], dts[args.vae_dtype]
    wseed = pkg.SEED_F16_WEIGHTS if args.weights == "f16" else 0      # (flag bit on the synthetic seed: parameters rounded to f16 on the device)

    ctx = pkg.Context(local_rank)
    cfg = pkg.sdxl_base_config()
    # rank 0 builds the weights; replicas allocate the identical arena and receive it over RCCL / xGMI
    t0 = time.time()
    diffuser = pkg.Diffuser(ctx, cfg, dt, seed=wseed | 0, empty=(rank != 0))
    decoder = pkg.LatentDecoder(ctx, None, vdt, seed=wseed | 0, with_encoder=(args.config == 5), empty=(rank != 0))      # (--weights f16: the VAE record is f16 too)
    refiner = None
    rcfg = pkg.sdxl_refiner_config()
    if args.config == 4:
        refiner = pkg.Diffuser(ctx, rcfg, dt, seed=wseed | 1, empty=(rank != 0))
    ctx.synchronize()
    # the MIX classes in force: an f32_split_mix_f16w model on parameters that are not f16 values falls back to f32_split_mix's (the engine checks the
    # tensors).  Replicas are laid out for the mode itself, so a fallen-back root must not broadcast into them.
    mix_classes = diffuser.diffusion.mix_classes()
    if world > 1 and args.dtype.endswith(("f16w", "geglu2")) and args.weights != "f16":
        raise SystemExit("bench.py: --dtype f32_split_mix_f16w across ranks needs --weights f16 (rank 0 would fall back to f32_split_mix and its arena "
                         "would not match the replicas')")
    t_build = time.time() - t0
    t0 = time.time()
    bcast_path, rccl_ranks = None, 1
    if world > 1:
        # the library's schedule (scatter over the root's xGMI links + in-place all-gather) on its own communicator.  Which path
        # runs is decided COLLECTIVELY: a rank-local try/except would leave some ranks inside the library's RCCL calls while
        # others wait in torch.distributed.broadcast (a hang, not a fallback) -- so every stage ends in an all-reduced "ok" flag
        # and every rank takes the fallback if any rank failed.  The fallback re-broadcasts everything (idempotent).
        import torch.distributed as dist

        def all_ok(ok: bool) -> bool:
            t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(t.item())

        comm, err = None, None
        try:
            comm = make_comm(pkg, local_rank)
        except Exception as e:
            err = e
        ok = all_ok(comm is not None)
        stages = [lambda: comm.bcast_unet(diffuser.diffusion), lambda: comm.bcast_vae(decoder)]
        if refiner is not None:
            stages.append(lambda: comm.bcast_unet(refiner.diffusion))
        for st in stages:
            if not ok:
                break
            try:
                st()
                torch.cuda.synchronize()
                good = True
            except Exception as e:
                err, good = e, False
            ok = all_ok(good)
        if ok:
            bcast_path = "sdxl_*_bcast_weights (library RCCL communicator: scatter + all-gather)"
            rccl_ranks = world
        else:   # never lose a scaling run to the communicator: torch.distributed's RCCL broadcast instead, on every rank
            print(f"[bench] rank {rank}: library broadcast unavailable on some rank ({err}); all ranks fall back to torch.distributed.broadcast",
                  file=sys.stderr, flush=True)
            broadcast_arena(diffuser.diffusion.weight_arena_tensor())
            broadcast_arena(decoder.weight_arena_tensor())
            if refiner is not None:
                broadcast_arena(refiner.diffusion.weight_arena_tensor())
            bcast_path = "torch.distributed.broadcast (fallback)"
            rccl_ranks = world
        torch.cuda.synchronize()
    t_bcast = time.time() - t0
    if args.no_graph:
        diffuser.diffusion.set_graph(False)
    if args.split_cfg:
        diffuser.diffusion.set_split_cfg(True)
    if args.unfused_xattn:
        diffuser.diffusion.set_fused_cross_attention(False)
    diffuser.enable_step_timing(True)

    lat = res // 8
    iters = pkg.step_count(n_steps)
    r_iters = pkg.step_count(n_steps, 800) if args.config == 4 else 0

    npc = args.prompts_per_call
    if npc != 1 and args.config != 2:
        raise SystemExit("--prompts-per-call > 1 is defined for --config 2 only")

    def make_prompt(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
        kw = dict(context_full=r(npc, 77, cfg.context_dim), channel_context=r(npc, cfg.adm_in_channels),
                  unconditional_context_full=r(77, cfg.context_dim), unconditional_channel_context=r(cfg.adm_in_channels),
                  resolution=(res, res))
        if args.config == 4:
            kw.update(context_open_clip=r(1, 77, rcfg.context_dim), channel_context_refiner=r(1, rcfg.adm_in_channels),
                      unconditional_context_open_clip=r(77, rcfg.context_dim),
                      unconditional_channel_context_refiner=r(rcfg.adm_in_channels))
        extra = {}
        if args.config == 4:
            extra["refine_noise"] = r(1, 4, lat, lat)
        if args.config == 5:
            extra["image"] = (torch.rand(1, res, res, 3, device=dev, generator=g) * 255).to(torch.uint8)
            extra["step_noise"] = r(iters, 1, 4, lat, lat)
            m = torch.zeros(1, 4, lat, lat, dtype=torch.bool, device=dev)
            m[:, :, 0:200 // 8, :] = True          # README: crop rows 0..200 px -> latent rows 0..25 (sample/main.rs:164-169)
            extra["mask"] = m
        return pkg.Conditioning(**kw), r(npc, 4, lat, lat), extra

    # throughput pipelining (serving shape): latent_to_image of image i runs on a second HIP stream while the UNet steps of
    # image i+1 start on the sampling stream -- the f32 VAE is matrix-pipe bound, the batch-2 UNet step leaves CUs idle.
    # Every image's full work (sampling + decode) still completes inside the timed region (device-wide synchronize).
    pipelined = args.pipeline_decode and args.config != 5      # config 5 encodes and decodes through ONE Vae handle
    dec_stream = torch.cuda.Stream() if pipelined else None

    def decode(latent):
        if not pipelined:
            return decoder.latent_to_image(latent)
        ev = torch.cuda.Event()
        ev.record()                      # legacy default stream: ordered behind the engine's (blocking) sampling stream
        dec_stream.wait_event(ev)
        latent.record_stream(dec_stream)
        with torch.cuda.stream(dec_stream):
            return decoder.latent_to_image(latent)

    def one_image(p):
        cond, noise, extra = p
        if args.config == 5:
            ref_latent = decoder.image_to_latent(pkg.RawImages(extra["image"], res, res))
            latent = diffuser.sample_latent_with_inpainting(cond, cfg_scale, n_steps, ref_latent, extra["mask"], noise, extra["step_noise"])
        else:
            latent = diffuser.sample_latent(cond, cfg_scale, n_steps, noise)
        if args.config == 4:
            latent = refiner.refine_latent(latent, cond, cfg_scale, 800, n_steps, extra["refine_noise"])   # sample/main.rs:262
        return latent, decode(latent)

    prompts_ready = [make_prompt(prompt_seed(rank, s)) for s in range(-args.warmup, args.steps)]   # resident before timing
    step_ms = []
    for w in range(args.warmup):
        one_image(prompts_ready[w])
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.steps):
        latent, last = one_image(prompts_ready[args.warmup + s])
        step_ms += diffuser.step_times_ms()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = max_over_ranks(time.perf_counter() - t0, dev)
    finite = bool(torch.isfinite(latent).all().item())
    n_images = sum_over_ranks(float(args.steps * npc), dev)

    # what the last timed image returned to its caller, written after the timed region
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"latent": latent, "image": last.buffer})

    sc = (res / 1024.0) ** 2
    # SURVEY section 8(d) gives exact counts at 1024^2 and 512^2 (attention is quadratic in the pixel count); other sizes scale by area
    fwd_tf = {1024: TFLOP_PER_UNET_FWD_1024, 512: TFLOP_PER_UNET_FWD_512}.get(res, TFLOP_PER_UNET_FWD_1024 * sc)
    dec_tf = {1024: TFLOP_VAE_DECODE_1024, 512: TFLOP_VAE_DECODE_512}.get(res, TFLOP_VAE_DECODE_1024 * sc)
    tflop_image = iters * 2 * fwd_tf + dec_tf
    if args.config == 4:
        tflop_image += r_iters * TFLOP_REFINER_FWD_1024 * sc
    if args.config == 5:
        tflop_image += dec_tf                            # encoder ~ mirror of the decoder
    value = n_images / elapsed

    # --full: measurements that take runs of their own (null on the line of a plain run)
    decode_ms, roofline = None, None
    if args.full:
        # decode leg on its own (outside the timed region): ms per latent_to_image at this resolution and VAE precision
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(3):
            decoder.latent_to_image(latent)
        e1.record()
        torch.cuda.synchronize()
        decode_ms = e0.elapsed_time(e1) / 3 / npc      # per image

        # --- roofline of the dominant kernel, measured live with hipEvents on the timed configuration (B=2 CFG pair)
        prof = diffuser.diffusion.profile(2 * npc, lat, lat)
        # The eager profile brackets every launch with two hipEvents, so its class times carry the events' own cost.  `frac` is computed from
        # those RAW times (a lower bound of the kernel's rate).  The overhead is calibrated DIRECTLY (round 6): the same eager chain is
        # timed once more without the per-launch events (one event pair around the whole forward, sdxl_unet_eager_forward_ms); (class sum - that) /
        # launches is what a bracketed launch carries, independent of what the captured graph gains elsewhere (warming workgroups, no host
        # launches).  The class times with that overhead removed are reported next to the raw ones as DERIVED figures; they sum to the un-bracketed
        # eager forward, not -- by construction -- to the graph-replayed step (r5 booked the whole eager-vs-graph gap as event overhead).
        p50_all = statistics.median(step_ms) if step_ms else None
        raw_ms = {k: float(v[0]) for k, v in prof.items()}
        n_launch = {k: int(v[1]) for k, v in prof.items()}
        class_sum = sum(raw_ms.values())
        eager_plain_ms = diffuser.diffusion.eager_forward_ms(2 * npc, lat, lat)
        ev_over_ms = 0.0
        if class_sum > eager_plain_ms > 0 and sum(n_launch.values()) > 0:
            ev_over_ms = (class_sum - eager_plain_ms) / sum(n_launch.values())
        adj_ms = {k: max(raw_ms[k] - n_launch[k] * ev_over_ms, 0.0) for k in raw_ms}
        ig_ms, ig_n, ig_fl = raw_ms["igemm"], prof["igemm"][1], prof["igemm"][2]
        # f32: exact-fp32 MFMA peak; f32_split: three f16 MFMAs per product -> a third of the f16 matrix peak in algorithmic FLOPs; the mixed modes run
        # one (f16 classes), two (split-operand classes on f16-representable weights) or three MFMAs per product: priced against the split peak for
        # f32_split_mix and against the full f16 peak for f32_split_mix_f16w (most of its FLOPs are single-MFMA classes) -- `peak_note` says so
        peak = PEAK_F32_TFLOPS if args.dtype == "f32" else (PEAK_F16_TFLOPS / 3.0 if args.dtype in ("f32_split", "f32_split_mix") else
                                                            PEAK_F16_TFLOPS / 2.0 if args.dtype == "f32_split_f16w" else PEAK_F16_TFLOPS)
        achieved = ig_fl / 1e12 / (ig_ms / 1e3) if ig_ms > 0 else 0.0
        achieved_adj = ig_fl / 1e12 / (adj_ms["igemm"] / 1e3) if adj_ms["igemm"] > 0 else 0.0
        # HBM-side traffic of the same launches: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/profile_step.py,
        # summarised by tools/pmc_traffic.py (gfx950 correction applied there); null when no committed summary exists
        traffic, traffic_src = None, None
        for tname in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
            tpath = os.path.join(ROOT, "profiles", tname)
            if os.path.exists(tpath) and args.dtype == "f16" and res == 1024:
                try:
                    with open(tpath) as fh:
                        traffic = round(json.load(fh)["igemm_total"]["bytes_per_launch"])
                    traffic_src = f"profiles/{tname} (bytes per implicit-GEMM launch, averaged over one UNet step)"
                    break
                except Exception:
                    traffic = None
        roofline = {"bound": "mfma", "kernel": "igemm_{pipe,glds}_kernel (NHWC implicit-GEMM conv3x3/1x1/linear, direct-to-LDS f16)",
                    "achieved": round(achieved, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                    "traffic": traffic, "traffic_source": traffic_src,
                    "peak_note": {"f32": "exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) dense peak", "f32_split": "f16 dense MFMA peak / 3 (three MFMAs per product)",
                                  "f32_split_mix": "f16 dense MFMA peak / 3 (split-operand classes: three MFMAs per product; two classes run one)",
                                  "f32_split_mix_f16w": "f16 dense MFMA peak; the eight f16 classes run one MFMA per product, the split-operand classes two on "
                                                        "f16-representable weights -- algorithmic TFLOP/s understate the matrix work of this mode",
                                  "f32_split_mix_f16w_geglu2": "f16 dense MFMA peak; as f32_split_mix_f16w with the GEGLU projection at two MFMAs per product",
                                  "f32_split_f16w": "f16 dense MFMA peak / 2 (two MFMAs per product on f16-representable weights)"}.get(args.dtype, "f16 dense MFMA peak of the MI355X"),
                    "launches_per_unet_step": ig_n, "avg_launch_us": round(1e3 * ig_ms / max(ig_n, 1), 2),
                    "algorithmic_tflop_per_unet_step": round(ig_fl / 1e12, 3),
                    # headline class times = the RAW event-bracketed ones (frac / achieved follow them); derived: the same with the calibrated event overhead removed
                    "class_ms_per_unet_step": {k: round(v, 3) for k, v in raw_ms.items()},
                    "class_sum_ms": round(class_sum, 3),
                    "eager_forward_ms_without_events": round(eager_plain_ms, 3),
                    "event_overhead_us_per_launch": round(1e3 * ev_over_ms, 3),
                    "class_ms_event_overhead_removed": {k: round(v, 3) for k, v in adj_ms.items()},
                    "frac_event_overhead_removed": round(achieved_adj / peak, 4),
                    "class_method": "eager pass with hipEvents around every launch (raw: frac / achieved / class_ms_per_unet_step); event overhead per launch = "
                                    "(raw class sum - the same eager chain timed WITHOUT per-launch events) / launches, removed in the *_event_overhead_removed figures; "
                                    "the graph-replayed step (unet_step_ms_p50) additionally gains from weight-warming workgroups and the absence of host launches",
                    # the whole CFG step against the peak (2 UNet forwards = SURVEY 8d's 13.52 TFLOP at 1024^2 over the graph-replayed step p50): attention, norms
                    # and every launch boundary included -- next to the GEMM-class fraction above
                    "whole_step_tflops": None if not p50_all else round(2 * npc * fwd_tf / (p50_all / 1e3), 1),
                    "whole_step_frac_of_peak": None if not p50_all else round(2 * npc * fwd_tf / (p50_all / 1e3) / peak, 4),
                    "whole_job_tflops": round(tflop_image * value, 1),
                    "whole_job_frac_of_peak": round(tflop_image * value / (peak * max(world, 1)), 4),
                    "flop_accounting": "tflop_per_image is the REFERENCE's count (SURVEY 8d); the engine hoists the cross-attention K/V "
                                       "projections out of the step (constant context), ~0.8 % fewer FLOPs executed than credited"}

    if rank == 0:
        cpu = None
        if args.full and not args.no_cpu_baseline and world == 1:
            if args.config == 1:
                cpu, _ = cpu_oracle_config1()
            else:
                cpu = cpu_baseline(res)
                if args.config != 2:    # extrapolate by this config's FLOPs instead of configs[1]'s
                    cpu["value"] = cpu["tflops"] / tflop_image
                    cpu["sample"] += f"; rescaled to this config's {tflop_image:.1f} TFLOP per image"
        p50 = statistics.median(step_ms) if step_ms else None
        # `live` (and `strict_f32`) are measured in THIS run; `committed_report` is the static summary of the parity tests' last
        # recorded run under profiles/ -- context, not a measurement of this run
        committed, strict = (load_parity() if args.full else None), None
        parity = {"committed_report": committed} if committed else None
        if args.full and args.config == 2 and res == 1024 and world == 1 and npc == 1 and not args.no_live_parity:
            try:
                live, strict = live_parity(pkg, ctx, diffuser, decoder, args.dtype, args.vae_dtype, args.weights)
                parity = dict(parity or {}, **{"live": live})
            except Exception as e:      # a missing fixture must not cost the bench line; say so on the line
                parity = dict(parity or {}, **{"live": {"error": repr(e)}})
        wl = (f"SDXL-base {res}x{res}, n_steps={n_steps} ({iters} CFG UNet step pairs), CFG {cfg_scale}, batch 1 prompt/GPU + VAE decode "
              f"to u8 ({C['label']})")
        if npc > 1:
            wl = wl.replace("batch 1 prompt/GPU", f"{npc} independent prompts per call (UNet batch {2 * npc}) -- NOT BASELINE.json's batch-1 configuration")
        out = {
            "metric": "images/sec SDXL-base 1024x1024 30-step CFG7.5 (whole job); UNet step ms p50",
            "value": round(value, 4), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": {"f32": "f32", "f32_split": "f32 (split f16 operands)", "f32_split_mix": "f32 (split f16 operands; self-attention and GEGLU projection on plain f16)",
                                           "f32_split_mix_f16w": "f32 stream, split f16 operands in the convolutions / cross-attention, eight transformer classes on plain f16",
                                           "f32_split_mix_f16w_geglu2": "f32 stream, split f16 operands in the convolutions / cross-attention / GEGLU activations, seven transformer classes on plain f16",
                                           "f32_split_f16w": "f32 (split f16 operands, two MFMAs per product on f16-representable weights)"}.get(args.dtype, "f16"), "data": "synthetic",
            "config": {"workload": wl, "baseline_config_index": args.config - 1,
                       "precision": args.dtype, "vae_dtype": args.vae_dtype,
                       "weights": "synthetic seeded (random-init SDXL-base architecture)" + (", every parameter rounded to IEEE f16 (what the reference's records hold)" if args.weights == "f16" else ""),
                       "mix_classes": mix_classes,
                       "parallelism": f"replica x{world}, 1 prompt per GPU, weights broadcast once over RCCL",
                       "hipgraph": not args.no_graph, "split_cfg": bool(args.split_cfg), "fused_xattn": not args.unfused_xattn,
                       "pipelined_decode": bool(pipelined), "prompts_per_call": npc, "full": bool(args.full),
                       # which build of the engine ran (SDXL_LIB_PATH / SDXL_MEASURE_LIB swap it: tools only) and the A/B knobs in force
                       "library": os.path.relpath(pkg.LIB_PATH, ROOT), "debug_set": os.environ.get("SDXL_DEBUG_SET", "")},
            "images_per_sec_per_gpu": round(value / world, 4),
            "unet_step_ms_p50": None if p50 is None else round(p50, 3),
            "vae_dtype": args.vae_dtype, "decode_ms": None if decode_ms is None else round(decode_ms, 2),
            "tflop_per_image": round(tflop_image, 1),
            "outputs_finite": finite,
            "setup_s": {"build_weights": round(t_build, 2), "broadcast": round(t_bcast, 2), "broadcast_path": bcast_path},
            "rccl_ranks": rccl_ranks,
            "roofline": roofline,
            "cpu_baseline": cpu,
            "parity": parity,
            "strict_f32": strict,
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
