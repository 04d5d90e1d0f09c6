"""Event-timed medians of masked (inpaint) sampling on the GPU: DiffusionRunner.sample, 8 views x 20 euler steps at 64 x 64
latents (512^2 pixels), cfg 7.5 (batch 16), hipGraph replay, SD1.x UNet on seeded synthetic weights in fp16, with a noise_mask and
without one.

  unmasked       sample(noise, 20, "euler", "normal", latent_image=...)
  masked         the same call with noise_mask = one feathered 512 x 512 mask on the device (prepare_mask's resize to 64 x 64 is part
                 of the call): two more launches per model evaluation (sr_inp_blend_in, sr_inp_blend_out) and a workspace latent
  floor          what those two launches cannot beat: their bytes (blend_in reads x, noise, latent_image and the mask and writes the
                 workspace; blend_out reads den, latent_image, x and the mask and writes den and d) / 8 TB/s of HBM + 2 us per launch
                 boundary, per step and per call
  parent         with --parent PATH (a checkout of the commit before this feature, its native libraries built): its unmasked call in
                 processes of its own, alternating with this tree's (parent, this, parent, this), so that the two medians can be held
                 against the spread between two runs of the same code

The two variants of one tree alternate call by call inside one process.  Per variant: warm-up, then the median of `runs` single calls
timed with events (min, max and the quartiles beside it).

    python tools/bench_inpaint.py [--runs 50] [--parent PATH] [--out profiles/inpaint_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S, LAUNCH_S = 8.0e12, 2.0e-6
N, H, W, STEPS, CFG = 8, 64, 64, 20, 7.5


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), q1_ms=q[0], q3_ms=q[2], runs=len(ms))


def child(repo, runs, masked):
    """one process, one tree: -> {"unmasked": stats, "masked": stats}"""
    sys.path.insert(0, repo)
    import torch
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from stable_renderer_amd import synth
    from stable_renderer_amd.model_shapes import unet_names_shapes
    from stable_renderer_amd.sampling import DiffusionRunner
    from stable_renderer_amd.unet import UNet, SD15_CFG
    ns, norms = unet_names_shapes(SD15_CFG)
    net = UNet(synth.synth_state_dict(ns, seed=0, norm_names=norms), SD15_CFG, dtype=torch.float16)
    g = torch.Generator().manual_seed(1)
    noise, pos, neg = torch.randn(N, 4, H, W, generator=g), torch.randn(1, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g)
    lat = torch.randn(N, 4, H, W, generator=g) * 5.0
    ys, xs = torch.arange(8 * H, dtype=torch.float32)[:, None], torch.arange(8 * W, dtype=torch.float32)[None, :]
    dist = torch.maximum((ys - 4 * H).abs() / (2.4 * H), (xs - 4 * W).abs() / (2.4 * W))
    mask = torch.clamp((1.35 - dist) / 0.7, 0.0, 1.0)[None].cuda()                   # (1, 512, 512): a feathered box
    run = DiffusionRunner(net, N, H, W, CFG, use_graph=True)
    run.set_conditioning(pos, neg)
    variants = {"unmasked": {}}
    if masked:
        variants["masked"] = {"noise_mask": mask}
    times = {k: [] for k in variants}
    outs = {}
    for it in range(3 + runs):                                                   # three warm-up rounds, then the timed ones
        for k, kw in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out, _ = run.sample(noise, STEPS, "euler", "normal", seed=0, latent_image=lat, **kw)
            b.record()
            b.synchronize()
            if it >= 3:
                times[k].append(a.elapsed_time(b))
            outs[k] = out
    res = {k: stats(v) for k, v in times.items()}
    if masked:                                                                   # a sanity check of what is timed; the tests hold the bounds
        keep = (torch.nn.functional.interpolate(mask[None], size=(H, W), mode="bilinear") == 0).expand(N, 4, H, W)
        res["kept_region_max_abs_diff"] = float((outs["masked"] - lat.cuda())[keep].abs().max())
        res["masked_vs_unmasked_max_abs_diff"] = float((outs["masked"] - outs["unmasked"]).abs().max())
        assert res["kept_region_max_abs_diff"] < 1e-3 < res["masked_vs_unmasked_max_abs_diff"]
    return res


def spawn(repo, runs, masked):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repo", repo, "--runs", str(runs)] + ([] if masked else ["--unmasked-only"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d):\n%s" % (r.returncode, r.stderr[-3000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def floor():
    lat_b, mask_b = N * 4 * H * W * 4, H * W * 4
    nbytes = (3 * lat_b + mask_b + lat_b) + (3 * lat_b + mask_b + 2 * lat_b)
    per_step = nbytes / HBM_BYTES_PER_S + 2 * LAUNCH_S
    return dict(bytes_per_step=nbytes, floor_us_per_step=per_step * 1e6, floor_us_per_call=per_step * STEPS * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--parent", default=None, help="a built checkout of the commit before this feature")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_bench.json"))
    ap.add_argument("--repo", default=ROOT)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--unmasked-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.repo, a.runs, not a.unmasked_only)))
        return
    order = [("this", ROOT, True)]
    if a.parent:
        order = [("parent", a.parent, False), ("this", ROOT, True), ("parent", a.parent, False), ("this", ROOT, True)]
    rounds = []
    for label, repo, masked in order:
        r = spawn(repo, a.runs, masked)
        rounds.append(dict(tree=label, **r))
        print("%-7s unmasked %8.2f ms (%.2f .. %.2f)" % (label, r["unmasked"]["median_ms"], r["unmasked"]["min_ms"], r["unmasked"]["max_ms"]) +
              ("   masked %8.2f ms (%.2f .. %.2f)" % (r["masked"]["median_ms"], r["masked"]["min_ms"], r["masked"]["max_ms"]) if masked else ""),
              flush=True)
    mine = [r for r in rounds if r["tree"] == "this"]
    over = [r["masked"]["median_ms"] - r["unmasked"]["median_ms"] for r in mine]
    res = dict(workload=f"{N} views x {STEPS} euler steps, {8 * H} x {8 * W} pixels, cfg {CFG}, fp16 SD1.x UNet, hipGraph", rounds=rounds,
               masked_overhead_ms_per_call=over, masked_overhead_us_per_step=[o / STEPS * 1e3 for o in over], **floor())
    if a.parent:
        theirs = [r for r in rounds if r["tree"] == "parent"]
        res["unmasked_medians_ms"] = dict(parent=[r["unmasked"]["median_ms"] for r in theirs], this=[r["unmasked"]["median_ms"] for r in mine])
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
