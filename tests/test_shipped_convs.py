"""CPU side of the shipped (conv geometry, kernel) pairs (tests/shipped_convs.py): the enumeration cannot shrink
unseen, the record decoder round-trips, and the fp32 bounds reject a lost partial product on every generated case, so
that test_shipped_convs_gpu.py holding a kernel to them means what the REFERENCE rows mean for the listed cases.
"""
from __future__ import annotations

import pytest
import torch

import fp32_bounds as fb
import shipped_convs as sc


def test_decode_conv_round_trips_a_record():
    from inference_arena_amd.engine import planner as P

    b = P.ProgramBuilder("fp32")
    src, dst, res, up = b.tensor("x", 12, 12, 96), b.tensor("y", 12, 12, 160), b.tensor("r", 12, 12, 192), \
        b.tensor("u", 24, 24, 224)
    w, bias = torch.zeros(80, 40, 3, 3), torch.zeros(80)
    b.conv(P.View(src, 16, 40), P.View(dst, 32, 80), w, bias, stride=1, pad=(1, 1), act="relu6",
           res=P.View(res, 48, 80), dst2=P.View(up, 64, 80), kind=P.CROPS)
    rec = b.ops[-1]
    d = P.ProgramBuilder.decode_conv(rec)
    want = dict(x_buf=src.id, x_coff=16, x_cs=96, H=12, W=12, Cin=40, Kpad=368, y_buf=dst.id, y_coff=32, y_cs=160, Ho=12,
                Wo=12, Cout=80, Cout_pad=80, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, res_buf=res.id, res_coff=48,
                res_cs=192, y2_buf=up.id, y2_coff=64, y2_cs=224, act=P.ACT["relu6"], f32out=0, batch_kind=P.CROPS,
                pw_cout=0, has_w3=1, f32=1)
    assert {k: d[k] for k in want} == want
    assert [P.OP_CONV] + [d[n] for n in P.CONV_FIELDS] == list(rec[:1 + len(P.CONV_FIELDS)])
    assert len(P.CONV_FIELDS) == 41 and not any(rec[1 + len(P.CONV_FIELDS):P.OP_DTYPE_FIELD])
    g = sc.geometry_of(rec)
    assert (g.src, g.dst, g.res, g.dst2, g.res_in_dst) == (sc.Slice(True, 16, 96), sc.Slice(True, 32, 160),
                                                           sc.Slice(True, 48, 192), sc.Slice(True, 64, 224), False)
    assert (g.act, g.pw, g.f32out, g.dtype) == ("relu6", None, False, "fp32")

    # out_hw, asymmetric use of the padding, a fused 1x1 without a stored 3x3 result, bf16
    b = P.ProgramBuilder("bf16")
    s2d, o = b.tensor("s", 10, 10, 16), b.tensor("o", 10, 10, 32)
    b.conv(P.View(s2d, 0, 16), P.View(o, 0, 32), torch.zeros(32, 16, 2, 2), torch.zeros(32), pad=(1, 1), out_hw=(10, 10),
           act=None, f32out=True)
    d = P.ProgramBuilder.decode_conv(b.ops[-1])
    assert (d["Ho"], d["Wo"], d["pad_t"], d["pad_l"], d["KH"], d["act"], d["f32out"], d["f32"], d["res_buf"]) == \
        (10, 10, 1, 1, 2, 0, 1, 0, P.BUF_NONE)
    g = sc.geometry_of(b.ops[-1])
    assert sc.out_hw(g, 10) == 10 and sc.out_hw(g, 32) == 32 and not g.res.present and not g.dst2.present
    head = b.tensor("h", 10, 10, 144)
    b.conv(P.View(o, 0, 32), P.View(P.BUF_NONE, 0, 64), torch.zeros(64, 32, 3, 3), torch.zeros(64),
           pw=(torch.zeros(48, 64, 1, 1), torch.zeros(48), P.View(head, 64, 48), None))
    d = P.ProgramBuilder.decode_conv(b.ops[-1])
    assert (d["y_buf"], d["pw_cout"], d["pw_cout_pad"], d["pw_kpad"], d["pw_y_buf"], d["pw_y_coff"], d["pw_y_cs"],
            d["pw_act"]) == (P.BUF_NONE, 48, 48, 64, head.id, 64, 144, 0)
    g = sc.geometry_of(b.ops[-1])
    assert not g.dst.present and g.pw == (48, sc.Slice(True, 64, 144), None)
    with pytest.raises(ValueError):
        P.ProgramBuilder.decode_conv([P.OP_DWCONV] + [0] * 47)


def test_reduced_maps_keep_the_tile_remainders():
    assert [sc.reduced_hw(h) for h in (1, 7, 14, 20, 24, 40, 80, 112, 160, 320)] == [1, 7, 14, 20, 24, 24, 32, 32, 32, 32]
    for h in range(1, 400):
        r = sc.reduced_hw(h)
        assert r <= h and r % 16 == h % 16 and (h <= 24 or 17 <= r <= 32)


def test_enumeration_covers_every_conv_of_every_program():
    pairs, programs, uses = sc.enumerate_shipped()
    assert len(programs) == 14
    missing = [k for k, (_, buckets) in programs.items() if not buckets]
    assert not missing, f"no table entry matches {missing}: regenerate data/tuning/conv_tuning.json"
    for (name, dtype), (n_convs, buckets) in programs.items():
        assert n_convs > 0, (name, dtype)
        for b in buckets:
            ops = uses[(name, dtype, b)]
            assert len(ops) == n_convs and len({i for i, _, _ in ops}) == n_convs, (name, dtype, b)
            assert all((name, dtype, b) in pairs[g][impl] for _, g, impl in ops), (name, dtype, b)
    n32, n16 = sc.pair_count("fp32"), sc.pair_count("bf16")
    print(f"shipped conv pairs: fp32 {n32} over {len(sc.geometries('fp32'))} geometries, "
          f"bf16 {n16} over {len(sc.geometries('bf16'))} geometries")
    assert n32 >= 200, n32
    assert n16 >= 40, n16
    ids = [g.id for g in sc.geometries()]
    assert len(set(ids)) == len(ids), "two geometries share a test id"
    assert len(sc.REFUSES_REDUCED) <= 0.10 * (n32 + n16)
    keys = {sc.refusal_key(g, i) for g, impls in pairs.items() for i in impls}
    assert set(sc.REFUSES_REDUCED) <= keys, sorted(set(sc.REFUSES_REDUCED) - keys)


FP32 = sc.geometries("fp32")


def _z(geo, case, got):
    ref, var, _ = case.refs()
    h, w = sc.case_hw(geo, case)
    return fb.zstats(got[..., :h, :w], ref[..., :h, :w], var[..., :h, :w])


@pytest.mark.parametrize("geo", FP32, ids=[g.id for g in FP32])
def test_bounds_reject_a_lost_product_on_every_generated_case(geo):
    """What a REFERENCE row records for a listed case, asserted for a generated one: plain fp32 passes both tiers of
    the case's family, the x3 emulation without any one of its three small products fails both."""
    case = sc.fp32_case(geo)
    assert case.family == ("silu" if geo.pw is not None else "one")
    assert case.key not in fb.REFERENCE
    zmax, zrms = fb.ZMAX[case.family], fb.ZRMS[case.family]
    mx, rms = _z(geo, case, case.run32("torch"))
    print(f"FP32Z-CPU {geo.id} torch max_z {mx:.3f} rms_z {rms:.4f}")
    assert mx <= zmax and rms <= zrms, (mx, rms)
    for t in fb.SMALL:
        mx, rms = _z(geo, case, case.run32("x3", {"drop": (t,)}))
        print(f"FP32Z-CPU {geo.id} drop {t} max_z {mx:.3f} rms_z {rms:.4f}")
        assert mx > zmax and rms > zrms, (t, mx, rms)


@pytest.mark.parametrize("k", [3, 1])
def test_max_tier_rejects_a_localized_loss(k):
    """One product lost only from the last partial 16-pixel tile's columns on, or only in the last partial 32-deep K
    chunk: the max tier fails."""
    geo = next(g for g in FP32 if g.KH == k and g.Cin % 32 and sc.out_hw(g, sc.reduced_hw(g.H)) % 16
               and g.pw is None)
    case = sc.fp32_case(geo)
    wo = sc.case_hw(geo, case)[1]
    for dmg in ({"drop": ("mm",), "cols": wo // 16 * 16}, {"drop": ("mm",), "chans": geo.Cin // 32 * 32}):
        mx, rms = _z(geo, case, case.run32("x3", dmg))
        print(f"FP32Z-CPU {geo.id} {dmg} max_z {mx:.3f} rms_z {rms:.4f}")
        assert mx > fb.ZMAX[case.family], (dmg, mx)


BF16_PW = [g for g in sc.geometries("bf16") if g.pw is not None]


@pytest.mark.parametrize("geo", BF16_PW, ids=[g.id for g in BF16_PW])
def test_bf16_fused_pointwise_tiers_reject_damage(geo):
    """shipped_convs.assert_bf16_pw on the CPU emulation of conv3x3_v3.hip's fused 3x3 -> 1x1: the emulation passes,
    also when its sums run in another order (a channels-last input); an intermediate stored one bf16 step off
    where nothing sits next to a tie fails tier 2, and so does a 1x1 bias off by 2^-7 of itself on 16 channels,
    which tier 1 accepts."""
    import torch.nn.functional as F
    import bf16_bounds as bb

    d = sc.bf16_case(geo)
    x, conv, pw, refs = d["x"], (d["w"], d["b"]), (d["w2"], d["b2"]), d["refs"]
    emu = sc.pw_emulate(x, conv, pw)
    rms_ref = bb.fused_stats(emu, refs[2], refs[3])[1]
    fig = sc.assert_bf16_pw(emu, refs, rms_ref, "emulation")
    print(f"BF16PW-CPU {geo.id} " + " ".join(f"{k} {v:.4g}" for k, v in fig.items()))
    other = sc.pw_emulate(x.contiguous(memory_format=torch.channels_last), conv, pw)
    sc.assert_bf16_pw(other, refs, rms_ref, "emulation, channels-last sums")

    T = bb.bf(F.silu(F.conv2d(x.float(), bb.bf(conv[0]), conv[1].float(), padding=1)))
    w2 = bb.bf(pw[0])
    off = T.clone()
    off[:, 0] += bb.ulp_bf16(T[:, 0]).float() * (T[:, 0] != 0)   # channel 0 of every pixel: the next bf16 value up
    with pytest.raises(AssertionError, match="tier 2"):
        sc.assert_bf16_pw(F.conv2d(off, w2, pw[1].float()).to(torch.bfloat16), refs, rms_ref, "one step off")
    b2 = pw[1].float().clone()
    b2[:16] *= 1.0 + 2.0 ** -7
    with pytest.raises(AssertionError, match="tier [23]"):
        sc.assert_bf16_pw(F.conv2d(T, w2, b2).to(torch.bfloat16), refs, rms_ref, "scaled bias tile")
