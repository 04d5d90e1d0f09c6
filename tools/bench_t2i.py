"""Event-timed medians of the T2I-Adapter on the GPU, on the seeded synthetic weights of tests/t2i_ref.py.

  forward        T2IAdapter.build(...)["run"](hint): hint packing, every convolution and pooling, and the hand-over of the four maps to
                 the control buffers (copies = 2), for N = 8 (the frame loop's views) and N = 1:
                   SD1.x full width (320 / 640 / 1280 / 1280) at a 512^2 hint, ksize 1 (avg-pool, cin 64) and ksize 3 (stride-2 convs, cin 192)
                   the XL adapter (cin 256, ksize 1) at a 1024^2 hint
                 in TF/s of the network's FLOPs (2 k^2 Cin Cout H W per convolution)
  torch          the same network stated in PyTorch (tests/t2i_ref.TorchAdapter) on the same GPU in the same process: fp16 channels_last,
                 forward only, under torch.no_grad(), from the unshuffled hint's NCHW fp16 tensor
  floor          (packed weights + every activation read and written once, in bytes) / 8 TB/s of HBM + 2 us per launch boundary: what
                 a memory-bound evaluation of the same launch list cannot beat
  call           DiffusionRunner.sample, 8 views x 20 euler steps at 64 x 64 latents, cfg 7.5 (batch 16), hipGraph replay, on the same
                 commit in three variants: no control; one depth T2I-Adapter (a new hint every call, as a render-then-diffuse loop
                 brings one); one depth ControlNet

Per case: warm-up, then the median of `runs` single calls timed with events (min and max beside it).

    python tools/bench_t2i.py [--runs 50] [--call-runs 10] [--out profiles/t2i_bench.json] [--skip-call]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S, LAUNCH_S = 8.0e12, 2.0e-6


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--call-runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t2i_bench.json"))
    ap.add_argument("--skip-call", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    import t2i_ref as TR
    from stable_renderer_amd import t2i_adapter as TA
    rows = []
    configs = [("sd1 ksize1 avgpool", dict(channel=320, cin=64, ksize=1, use_conv=False), 512, 64),
               ("sd1 ksize3 conv", dict(channel=320, cin=192, ksize=3, use_conv=True), 512, 64),
               ("xl ksize1", dict(channel=320, cin=256, ksize=1, use_conv=False), 1024, 128)]
    with torch.no_grad():
        for label, case, px, lat in configs:
            sd = TR.synth_state_dict(seed=7, **case)
            ad = TA.T2IAdapter(sd)
            ref16 = TR.TorchAdapter(sd).cuda().eval().half().to(memory_format=torch.channels_last)
            r = ad.unshuffle_amount
            for N in (8, 1):
                hint = torch.rand(N, 3, px, px, generator=torch.Generator().manual_seed(N)).cuda()
                p = ad.build(2 * N, lat, lat, n_hints=N)
                p["run"](hint)
                bufs, ops, feats = ad.layer_plan(N, px // r, px // r)
                flops = sum(2 * L["ksize"] ** 2 * L["Cin"] * L["Cout"] * L["H"] * L["W"] * N for k, L, *_ in ops if k == "conv")
                nbytes = sum(2 * w.numel() for w, _ in ad.host.values())
                for op in ops:
                    if op[0] == "conv":
                        L = op[1]
                        nbytes += 2 * N * (L["Hs"] * L["Ws"] * L["Cin"] + L["H"] * L["W"] * L["Cout"] * (2 if L["res"] else 1))
                    else:
                        hs, ws, c = bufs[op[1]]
                        nbytes += 2 * N * c * (hs * ws + bufs[op[2]][0] * bufs[op[2]][1])
                launches = len(ops) + 1 + 4
                floor_ms = (nbytes / HBM_BYTES_PER_S + launches * LAUNCH_S) * 1e3
                mean_in = hint.mean(1, keepdim=True) if ad.channels_in == 1 else hint
                x16 = mean_in.half().contiguous(memory_format=torch.channels_last)
                want = ref16(x16)
                err = max(float((t.reshape(N, bufs[f][0], bufs[f][1], bufs[f][2]).permute(0, 3, 1, 2).float() - w_.float()).abs().max())
                          for t, f, w_ in zip(p["features"], feats, want))
                print(f"{label} N = {N}: max |native - torch fp16| = {err:.2e} over the four maps", flush=True)
                assert err < 0.25                                           # a sanity check of what is timed; the tests hold the bounds
                med, lo, hi = timed(lambda: p["run"](hint), a.runs)
                tmed, tlo, thi = timed(lambda: ref16(x16), a.runs)
                row = dict(case=f"{label} N={N} hint {px}x{px}", native_ms=med, native_min_ms=lo, native_max_ms=hi, torch_fp16_ms=tmed,
                           torch_min_ms=tlo, torch_max_ms=thi, floor_ms=floor_ms, gflop=flops / 1e9, tflops=flops / (med * 1e-3) / 1e12,
                           launches=launches, bytes=nbytes, torch_over_native=tmed / med)
                rows.append(row)
                print("%-34s native %8.3f ms (%.3f .. %.3f)  torch fp16 %8.3f ms  floor %6.3f ms  %7.1f GFLOP  %6.1f TF/s  torch / native %.2f" %
                      (row["case"], med, lo, hi, tmed, floor_ms, flops / 1e9, row["tflops"], tmed / med), flush=True)
                del p
            del ref16, ad
            torch.cuda.empty_cache()

    if not a.skip_call:
        from stable_renderer_amd import synth
        from stable_renderer_amd.controlnet import ControlNet
        from stable_renderer_amd.model_shapes import controlnet_names_shapes, unet_names_shapes
        from stable_renderer_amd.sampling import DiffusionRunner
        from stable_renderer_amd.unet import UNet, SD15_CFG
        ns, norms = unet_names_shapes(SD15_CFG)
        net = UNet(synth.synth_state_dict(ns, seed=0, norm_names=norms), SD15_CFG, dtype=torch.float16)
        cns, cnorms = controlnet_names_shapes(SD15_CFG)
        N, h, w, steps = 8, 64, 64, 20
        g = torch.Generator().manual_seed(1)
        noise, pos, neg = torch.randn(N, 4, h, w, generator=g), torch.randn(1, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g)
        hints = [torch.rand(N, 3, 8 * h, 8 * w, generator=g).cuda() for _ in range(4)]
        adapter = TA.T2IAdapter(TR.synth_state_dict(seed=7, channel=320, cin=64, ksize=1, use_conv=False))
        variants = [("no control", lambda: []), ("one depth T2I-Adapter", lambda: [adapter]),
                    ("one depth ControlNet", lambda: [ControlNet(synth.synth_state_dict(cns, seed=20, norm_names=cnorms), SD15_CFG, dtype=torch.float16)])]
        for label, make in variants:
            nets = make()
            run = DiffusionRunner(net, N, h, w, 7.5, use_graph=True, controlnets=nets)
            run.set_conditioning(pos, neg)
            k = [0]

            def call():
                if nets:
                    k[0] += 1
                    run.set_control_hints([hints[k[0] % len(hints)]])
                run.sample(noise, steps, "euler", "normal", seed=0)
            med, lo, hi = timed(call, a.call_runs, warmup=2)
            row = dict(case=f"call 8 views x {steps} steps: {label}", call_ms=med, call_min_ms=lo, call_max_ms=hi, per_step_ms=med / steps)
            if nets and nets[0] is adapter:
                row["adapter_evaluations"] = adapter.evaluations
            rows.append(row)
            print("%-52s %9.2f ms (%.2f .. %.2f)  %7.3f ms per step" % (row["case"], med, lo, hi, med / steps), flush=True)
            del run, nets
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
