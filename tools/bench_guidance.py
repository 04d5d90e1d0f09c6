"""Event-timed medians of patched sampling on the GPU: DiffusionRunner.sample, 8 views x 20 euler steps at 64 x 64 latents
(512^2 pixels), cfg 7.5 (batch 16), hipGraph replay, SD1.x UNet on seeded synthetic weights in fp16, with and without the model_sampling
and cfg_function patches.

  unpatched      DiffusionRunner(...): sr_cfg_denoise after every model evaluation, one launch, as ever
  v_prediction   DiffusionRunner(..., model_sampling=ModelSamplingDiscrete("v_prediction")): sr_gd_denoise and sr_gd_cfg, two launches
  v_rescale      the same with cfg_function=("rescale", 0.7): sr_gd_denoise and sr_gd_rescale's two launches, three in all
  floor          what the added launches cannot beat: the bytes they move beyond sr_cfg_denoise's (which reads x and the two chunks and
                 writes den and d: five latents) / 8 TB/s of HBM + 2 us per added launch boundary, per step and per call.
                 v_prediction: sr_gd_denoise reads three latents and writes two, sr_gd_cfg reads three and writes two: five latents and
                 one launch more.  v_rescale: the statistics launch reads three latents, the apply launch reads three and writes two:
                 thirteen in all, eight latents and two launches more
  parent         with --parent PATH (a checkout of the commit before this feature, its native libraries built): its call in processes
                 of its own, alternating with this tree's (parent, this, parent, this), so that the two medians can be held against the
                 spread between two runs of the same code

The variants of one tree alternate call by call inside one process.  Per variant: warm-up, then the median of `runs` single calls timed
with events (min, max and the quartiles beside it).

    python tools/bench_guidance.py [--runs 50] [--parent PATH] [--out profiles/guidance_bench.json]
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
ADDED = {"v_prediction": (5, 1), "v_rescale": (8, 2)}       # (latents moved, launches) beyond sr_cfg_denoise, per model evaluation


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), q1_ms=q[0], q3_ms=q[2], runs=len(ms))


def child(repo, runs, patched):
    """one process, one tree: -> {variant: stats}"""
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
    runners = {"unpatched": DiffusionRunner(net, N, H, W, CFG, use_graph=True)}
    if patched:
        from stable_renderer_amd import guidance as GDH
        ms = GDH.ModelSamplingDiscrete("v_prediction")
        runners["v_prediction"] = DiffusionRunner(net, N, H, W, CFG, use_graph=True, model_sampling=ms)
        runners["v_rescale"] = DiffusionRunner(net, N, H, W, CFG, use_graph=True, model_sampling=ms, cfg_function=("rescale", 0.7))
    for run in runners.values():
        run.set_conditioning(pos, neg)
    times = {k: [] for k in runners}
    outs = {}
    for it in range(3 + runs):                                                   # three warm-up rounds, then the timed ones
        for k, run in runners.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out, _ = run.sample(noise, STEPS, "euler", "normal", seed=0)
            b.record()
            b.synchronize()
            if it >= 3:
                times[k].append(a.elapsed_time(b))
            outs[k] = out
    res = {k: stats(v) for k, v in times.items()}
    if patched:                                                                  # a sanity check of what is timed; the tests hold the bounds
        assert all(bool(torch.isfinite(o).all()) for o in outs.values())
        res["v_vs_unpatched_max_abs_diff"] = float((outs["v_prediction"] - outs["unpatched"]).abs().max())
        res["rescale_vs_v_max_abs_diff"] = float((outs["v_rescale"] - outs["v_prediction"]).abs().max())
        assert res["v_vs_unpatched_max_abs_diff"] > 1e-3 and res["rescale_vs_v_max_abs_diff"] > 1e-3
    return res


def spawn(repo, runs, patched):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repo", repo, "--runs", str(runs)] + ([] if patched else ["--unpatched-only"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d):\n%s" % (r.returncode, r.stderr[-3000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def floor():
    lat_b = N * 4 * H * W * 4
    out = {}
    for k, (lats, launches) in ADDED.items():
        per_step = lats * lat_b / HBM_BYTES_PER_S + launches * LAUNCH_S
        out[k] = dict(added_bytes_per_step=lats * lat_b, added_launches_per_step=launches, floor_us_per_step=per_step * 1e6,
                      floor_us_per_call=per_step * STEPS * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--parent", default=None, help="a built checkout of the commit before this feature")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.json"))
    ap.add_argument("--repo", default=ROOT)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--unpatched-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.repo, a.runs, not a.unpatched_only)))
        return
    order = [("this", ROOT, True)]
    if a.parent:
        order = [("parent", a.parent, False), ("this", ROOT, True), ("parent", a.parent, False), ("this", ROOT, True)]
    rounds = []
    for label, repo, patched in order:
        r = spawn(repo, a.runs, patched)
        rounds.append(dict(tree=label, **r))
        print("%-7s " % label + "   ".join("%s %8.2f ms (%.2f .. %.2f)" % (k, v["median_ms"], v["min_ms"], v["max_ms"])
                                           for k, v in r.items() if isinstance(v, dict)), flush=True)
    mine = [r for r in rounds if r["tree"] == "this"]
    res = dict(workload=f"{N} views x {STEPS} euler steps, {8 * H} x {8 * W} pixels, cfg {CFG}, fp16 SD1.x UNet, hipGraph", rounds=rounds,
               floor=floor())
    for k in ADDED:
        over = [r[k]["median_ms"] - r["unpatched"]["median_ms"] for r in mine]
        res[k + "_overhead_ms_per_call"] = over
        res[k + "_overhead_us_per_step"] = [o / STEPS * 1e3 for o in over]
        res[k + "_ms_per_step"] = [r[k]["median_ms"] / STEPS for r in mine]
    if a.parent:
        theirs = [r for r in rounds if r["tree"] == "parent"]
        res["unpatched_medians_ms"] = dict(parent=[r["unpatched"]["median_ms"] for r in theirs], this=[r["unpatched"]["median_ms"] for r in mine])
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
