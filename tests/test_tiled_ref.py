"""Host half of the tiled VAE: the product's tile schedule against the tile lists recorded from the reference loop, the float64
restatement (tests/tiled_ref.py) against the reference's tiled output (tests/golden/vae_tiled.npz, tools/gen_golden_tiled.py), and
the argument errors.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import sr_oracle as O
import tiled_ref as TR
from stable_renderer_amd import synth, tiled

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEC = dict(h=13, w=22, tile=8, overlap=2)              # the fixture's shapes (tools/gen_golden_tiled.py)
ENC = dict(H=104, W=176, tile=64, overlap=16)


def _sd(keys, seed):
    with open(os.path.join(GOLD, keys)) as f:
        k = json.load(f)
    return synth.synth_state_dict([(n, tuple(s)) for n, s in k["names_shapes"]], seed=seed, norm_names=k["norm_names"])


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "vae_tiled.npz"))


def test_schedule_equals_reference_tile_lists(fix):
    dec = tiled.decode_passes(DEC["h"], DEC["w"], DEC["tile"], DEC["tile"], DEC["overlap"])
    enc = tiled.encode_passes(ENC["H"], ENC["W"], ENC["tile"], ENC["tile"], ENC["overlap"])
    shapes = set()
    for name, passes, up in (("dec", dec, 8.0), ("enc", enc, 0.125)):
        for i, (tiles, feather) in enumerate(passes):
            want = fix[f"{name}_tiles_{i}"].tolist()
            assert [list(t[:4]) for t in tiles] == want, (name, i)
            assert feather == round((DEC if name == "dec" else ENC)["overlap"] * up)
            for t in tiles:
                assert (t.oy, t.ox, t.oh, t.ow) == tuple(round(v * up) for v in t[:4])
            if name == "dec":
                shapes |= {(t.h, t.w) for t in tiles}
    assert sum(len(t) for t, _ in dec) == 37 and sum(len(t) for t, _ in enc) == 37
    assert len(shapes) == 13
    # the restatement's own loop lists the same tiles
    for (tx, ty), (tiles, _) in zip(((4, 16), (16, 4), (8, 8)), dec):
        assert TR.tiles_of(13, 22, tx, ty, 2, 8)[0] == [tuple(t[:4]) for t in tiles]


def test_schedule_lists_a_clamped_start_twice():
    tiles, feather = tiled.tile_schedule(5, 22, 4, 4, 3, 8)
    xs = [t.x for t in tiles if t.y == 0]
    assert xs == list(range(0, 19)) + [19, 19, 19] and feather == 24          # starts 19, 20, 21 all clamp to W - overlap = 19
    assert all(t.w == 4 for t in tiles[:19]) and tiles[21].w == 3


@pytest.mark.slow
def test_restatement_reproduces_reference_decode(fix):
    """measured max |restatement - reference| = 3.6e-07 on outputs up to 2.7 (the reference blends in fp32, the restatement in
    float64; the tile function is the same fp32 decoder); bound 5e-6"""
    sd = _sd("vae_dec_keys.json", 2)
    z = torch.randn(2, 4, 13, 22, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        out = TR.decode_tiled(z, lambda a: O.vae_decoder(sd, a), 8, 8, 2)
    err = np.abs(out - fix["dec_out"]).max()
    print("decode restatement vs reference: max abs diff %.3g, |ref| max %.3g" % (err, np.abs(fix["dec_out"]).max()))
    assert out.shape == (2, 3, 104, 176) and err < 5e-6, err


@pytest.mark.slow
def test_restatement_reproduces_reference_encode(fix):
    """measured max |restatement - reference| = 6.3e-07 on outputs up to 3.1; bound 5e-6.  The per-tile noise comes from the global generator in the
    reference's order: pass, image, y, x"""
    sd = _sd("vae_enc_keys.json", 3)
    pixels = torch.rand(2, 104, 176, 3, generator=torch.Generator().manual_seed(9))
    torch.manual_seed(31)
    with torch.no_grad():
        out = TR.encode_tiled(pixels.movedim(-1, 1), lambda a: O.vae_encode(sd, a.movedim(1, -1)), 64, 64, 16)
    err = np.abs(out - fix["enc_out"]).max()
    print("encode restatement vs reference: max abs diff %.3g, |ref| max %.3g" % (err, np.abs(fix["enc_out"]).max()))
    assert out.shape == (2, 4, 13, 22) and err < 5e-6, err


def test_draw_order_is_the_restatements():
    """tiled.draw_encode_noise consumes the global generator exactly as the per-tile encodes of the restatement do"""
    passes = tiled.encode_passes(ENC["H"], ENC["W"], 64, 64, 16)
    torch.manual_seed(31)
    drawn = tiled.draw_encode_noise(2, 4, passes)
    torch.manual_seed(31)
    k = 0
    for tx, ty in ((64, 64), (128, 32), (32, 128)):
        for _b in range(2):
            for _y, _x, h, w in TR.tiles_of(104, 176, tx, ty, 16, 1 / 8)[0]:
                assert torch.equal(drawn[k], torch.randn(1, 4, h // 8, w // 8))
                k += 1
    assert k == len(drawn) == 74


def test_tile_not_larger_than_overlap_is_an_error():
    with pytest.raises(ValueError):
        tiled.decode_passes(16, 16, 8, 8, 4)            # first pass: tile_x // 2 = 4 <= overlap
    with pytest.raises(ValueError):
        tiled.tile_schedule(16, 16, 8, 8, 8, 8)
    with pytest.raises(ValueError):
        tiled.encode_passes(128, 128, 64, 64, 32)       # tile_x // 2 = 32 <= overlap


def test_input_smaller_than_the_overlap_is_refused():
    """a deviation from the reference, which runs such an input through a mask loop that indexes the tile from its far end"""
    for H, W in ((8, 32), (32, 8)):
        with pytest.raises(ValueError):
            tiled.tile_schedule(H, W, 64, 64, 16, 8)
        with pytest.raises(ValueError):
            tiled.decode_passes(H, W)
    tiled.tile_schedule(16, 16, 64, 64, 16, 8)


def test_encode_tiles_must_map_onto_whole_latents():
    for tx, ty, ov in ((72, 64, 16), (64, 72, 16), (64, 64, 12)):
        with pytest.raises(ValueError):
            tiled.encode_passes(128, 128, tx, ty, ov)
    tiled.encode_passes(128, 128, 64, 64, 16)


def test_tiled_library_exports_every_declared_symbol():
    from stable_renderer_amd import _lib_tiled
    L = _lib_tiled.lib()                                   # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    assert len(_lib_tiled.SYMBOLS) == 6                    # == the header's declarations: test_abi.test_side_header_declares_exactly_its_table
    for name in _lib_tiled.SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.sr_tiled_source_hash()) == 32
    assert L.sr_tile_gather(None, None, 1, 1, 1, 0, 0, 1, 1, None) < 0 and b"sr_tile_gather" in L.sr_tiled_last_error()
