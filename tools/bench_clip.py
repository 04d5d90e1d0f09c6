"""Event-timed medians of the native CLIP text encoder on the GPU: clip-l (768 / 12 heads / 3072 / 12 layers, quick_gelu) and
clip-g (1280 / 20 / 5120 / 32 layers, gelu, penultimate layer, projected pooled row) with seeded synthetic weights, at R = 1, 2 and 8
sections of 77 tokens.

  native         ClipTextModel.forward: token processing on the host, three small uploads, sr_clip_embed and one sr_clip_run
  launches       the two native calls alone, on buffers already filled
  torch fp16     the same network written in plain PyTorch on the same GPU in the same process: fp16 parameters and activations,
                 F.layer_norm / F.linear / scaled_dot_product_attention(is_causal=True), under torch.no_grad()
  floor          what the encoder cannot beat as a chain of dependent launches: its matrix bytes (fp16, read once) over the 6.3 TB/s an
                 MI355X reaches on HBM, plus 1.45 us per dependent kernel boundary times the launch count

Per case: warm-up, then the median of `runs` single calls timed with events (min and max beside it).

    python tools/bench_clip.py [--runs 50] [--sections 1,2,8] [--out profiles/clip_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12                        # achievable HBM rate of one MI355X
BOUNDARY_S = 1.45e-6                            # one dependent kernel boundary on one stream
T, VOCAB = 77, 49408


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


def synth(cfg, seed, projection):
    """seeded fp16 CLIPTextModel weights, drawn on the GPU"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, FF = cfg["hidden_size"], cfg["intermediate_size"]
    lin = lambda n, k, gain=1.0: ((torch.rand(n, k, generator=g, device="cuda") * 2 - 1) * gain * (3.0 / k) ** 0.5).half()
    vec = lambda n, s=0.1: ((torch.rand(n, generator=g, device="cuda") * 2 - 1) * s).half()
    sd = {"text_model.embeddings.token_embedding.weight": (torch.randn(VOCAB, D, generator=g, device="cuda") * 0.5).half(),
          "text_model.embeddings.position_embedding.weight": (torch.randn(T, D, generator=g, device="cuda") * 0.5).half()}
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = (1.0 + vec(D, 0.3).float()).half(), vec(D)
        for n, gain in (("q_proj", 1.4), ("k_proj", 1.4), ("v_proj", 1.0), ("out_proj", 0.5)):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = lin(D, D, gain), vec(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = lin(FF, D), vec(FF)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = lin(D, FF, 0.5), vec(D)
    sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"] = (1.0 + vec(D, 0.3).float()).half(), vec(D)
    if projection:
        sd["text_projection.weight"] = lin(D, D)
    return sd


def torch_forward(sd, cfg, ids, inter, project):
    """the network in plain PyTorch, fp16 -> (hidden states of layer `inter` or the final-normed last layer, pooled)"""
    D, H, act = cfg["hidden_size"], cfg["num_attention_heads"], cfg["hidden_act"]
    R = ids.shape[0]
    x = sd["text_model.embeddings.token_embedding.weight"][ids] + sd["text_model.embeddings.position_embedding.weight"]
    mid = None
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        h = F.layer_norm(x, (D,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"])
        q, k, v = (F.linear(h, sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"]).view(R, T, H, 64).transpose(1, 2) for n in "qkv")
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(R, T, D)
        x = x + F.linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (D,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"])
        h = F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        h = h * torch.sigmoid(1.702 * h) if act == "quick_gelu" else F.gelu(h)
        x = x + F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        if i == inter:
            mid = x
    z = F.layer_norm(x, (D,), sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"])
    pooled = z[torch.arange(R, device=z.device), ids.argmax(-1)]
    if project:
        pooled = F.linear(pooled, sd["text_projection.weight"])
    return (z if mid is None else mid), pooled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--sections", default="1,2,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from stable_renderer_amd import _clip as K, clip as CL
    from stable_renderer_amd.ops import stream_ptr
    rows = []
    for name, cfg, special, opts, proj in (("clip-l", CL.CLIP_L, CL.SPECIAL_L, {}, False),
                                           ("clip-g", CL.CLIP_G, CL.SPECIAL_G, dict(layer="hidden", layer_idx=-2, layer_norm_hidden_state=False), True)):
        sd = synth(cfg, 1 if name == "clip-l" else 2, proj)
        model = CL.ClipTextModel(sd, cfg, special, **opts).to("cuda")
        inter = cfg["num_hidden_layers"] - 2 if opts else None
        for R in (int(v) for v in a.sections.split(",")):
            g = torch.Generator().manual_seed(R)
            tokens = []
            for r in range(R):
                n = 5 + (r * 23) % 70
                tokens.append([special["start"]] + torch.randint(1, 49000, (n,), generator=g).tolist() + [special["end"]] + [special["pad"]] * (T - 2 - n))
            ids = torch.tensor(tokens).cuda()
            with torch.no_grad():
                z, pooled = model.forward(tokens)
                tz, tp = torch_forward(sd, cfg, ids, inter, proj)
                ez, ep = float((z - tz.float()).abs().max()), float((pooled - tp.float()).abs().max())
                print(f"{name} R={R}: max |native - torch fp16| = {ez:.2e} (hidden, range {float(tz.max() - tz.min()):.1f}), {ep:.2e} (pooled)", flush=True)
                assert ez < 0.05 * float(tz.max() - tz.min())                 # a sanity check of what is timed; the tests hold the bounds
                arr, b, W = model._plan(R, False), model._buffers(R), model._dev[1]

                def launches():
                    K.check(K.lib().sr_clip_embed(b["ids"].data_ptr(), W["tok"].data_ptr(), None, W["pos"].data_ptr(), b["x"].data_ptr(), T * R, model.D,
                                                  model.vocab, 0, model.D, 0, stream_ptr()))
                    K.check(K.lib().sr_clip_run(arr, len(arr), stream_ptr()))
                nat = timed(lambda: model.forward(tokens), a.runs)
                lau = timed(launches, a.runs)
                tor = timed(lambda: torch_forward(sd, cfg, ids, inter, proj), a.runs)
            n_launch = len(arr) + 1
            floor = (model.weight_bytes() / HBM_BYTES_PER_S + n_launch * BOUNDARY_S) * 1e3
            row = dict(model=name, sections=R, runs=a.runs, native_ms=nat[0], native_min_ms=nat[1], native_max_ms=nat[2],
                       launches_ms=lau[0], launches_min_ms=lau[1], launches_max_ms=lau[2], torch_fp16_ms=tor[0], torch_fp16_min_ms=tor[1],
                       torch_fp16_max_ms=tor[2], launches=n_launch, weight_bytes=model.weight_bytes(), floor_ms=floor,
                       native_over_torch=tor[0] / nat[0], launches_over_floor=lau[0] / floor)
            rows.append(row)
            print("%-6s R=%d  native %7.3f ms (%.3f .. %.3f)  launches %7.3f ms  torch fp16 %7.3f ms (%.3f .. %.3f)  floor %.3f ms (%d launches, %.0f MB)"
                  "  torch / native %.2fx" % (name, R, *nat, lau[0], *tor, floor, n_launch, model.weight_bytes() / 1e6, tor[0] / nat[0]), flush=True)
        del model, sd
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")          # a row per line


if __name__ == "__main__":
    main()
