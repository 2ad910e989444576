"""GPU: ragged e2e / feedback attacks and ragged inference (avc_e2e_attack_ragged, avc_fb_attack_ragged,
avc_inference_ragged; Context.vc_attack_ragged / inference_ragged; batching.attack_many_ragged).

Real data gives vc_src, vc_tgt and adv_tgt three lengths per utterance (attack.py:41-56), so (T, T_src)
buckets hold one utterance each.  The ragged batch runs every component -- ContentEncoder, Decoder,
SpeakerEncoder(adv) and, for fb, SpeakerEncoder(decoder output) -- on the long engine, one launch per pass
over every length (per-workgroup lengths and packed offsets).  What it must equal: every utterance, bit for
bit, its own single-utterance attack with every component forced onto the long engine (the same kernels and
per-utterance arithmetic, the e2e loss mean and gradient scale over its own 80 x Tn elements); and through
that the reference's golden vectors and the float64 oracle at the bounds the long engine already holds.

The standard batch of (T, T_src): long utterances, the 128 / 129 boundaries of both lengths, the longest
source with T < T_src, and the shortest source the model accepts (17 frames: less than one chunk).  It runs
in two orders, so that the shortest and the longest utterance are each once the last block of every packed
buffer (nothing lies behind it for a clamped tail read to land on)."""
import copy

import numpy as np
import pytest
import torch

import attack_utils
import avc_native
import batching
from helpers import (TOL_GRAD_REL_VC, TOL_VC_GRAD_L2_MAX, TOL_VC_GRAD_L2_MEDIAN, cfg_of, check_adv, model_from_fixture,
                     rel)
from oracle import adain_vc as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (T, T_src); Tn = 8 ceil(T_src / 8)
STD = [(300, 280), (129, 136), (128, 128), (100, 129), (77, 600), (33, 17)]
ORDERS = {"shortest_last": [0, 1, 2, 3, 4, 5], "longest_last": [5, 0, 1, 2, 3, 4]}
FN = {"e2e": attack_utils.e2e_attack, "fb": attack_utils.fb_attack}


def _tn(ts):
    return 8 * ((ts + 7) // 8)


@pytest.fixture(scope="module")
def full(golden):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    z = golden("full_T128")
    m = model_from_fixture(z).to(DEV)
    ctx = avc_native.vc_context_for(m, DEV)
    yield z, m, ctx
    ctx.set_engine("auto")


def _utts(pairs, seed):
    """vc_src [80, T_src], vc_tgt / ptb0 [80, T], adv_tgt [80, max(40, T - 23)] per utterance."""
    g = torch.Generator().manual_seed(seed)
    src = [torch.randn(80, ts, generator=g).to(DEV) for _, ts in pairs]
    vc = [torch.randn(80, t, generator=g).to(DEV) for t, _ in pairs]
    at = [torch.randn(80, max(40, t - 23), generator=g).to(DEV) for t, _ in pairs]
    p0 = [torch.randn(80, t, generator=g).to(DEV) for t, _ in pairs]
    return src, vc, at, p0


@pytest.fixture(scope="module")
def std(full):
    z, m, ctx = full
    src, vc, at, p0 = _utts(STD, 21)
    te = torch.cat([ctx.se_forward(a[None]) for a in at])
    return src, vc, at, p0, te


def _single(ctx, kind, src, vc, p0, te, b, n, **kw):
    """utterance b's own attack, every component forced onto the long engine"""
    ctx.set_engine("long")
    try:
        adv, L, g0 = ctx.vc_attack(kind, src[b][None], vc[b][None], None, p0[b][None], 0.1, n, want_losses=True,
                                   want_grad0=True, tgt_emb=te[b:b + 1], **kw)
    finally:
        ctx.set_engine("auto")
    return adv[0], L[:, 0], g0[0]


def _pick(xs, order):
    return [xs[i] for i in order]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["e2e", "fb"])
def test_ragged_vc_equals_single_utterance_long(full, std, kind, prec):
    """55 iterations (one captured 50-iteration graph + 5 launches), both batch orders: adv, the loss history and
    grad0 of every utterance equal its own long-engine attack bitwise; a repeated call is bit-equal and builds,
    re-plans, captures and evicts nothing; |adv - vc| <= eps."""
    z, m, ctx = full
    src, vc, at, p0, te = std
    ref = [_single(ctx, kind, src, vc, p0, te, b, 55, precision=prec) for b in range(len(STD))]
    ctx.set_ws_cache(12)
    for name, order in ORDERS.items():
        args = (_pick(src, order), _pick(vc, order), te[order].contiguous(), _pick(p0, order))
        outs, L, g0 = ctx.vc_attack_ragged(kind, *args, 0.1, 55, precision=prec, want_losses=True, want_grad0=True)
        torch.cuda.synchronize()
        s1 = ctx.ws_stats()
        again, L2, _ = ctx.vc_attack_ragged(kind, *args, 0.1, 55, precision=prec, want_losses=True)
        torch.cuda.synchronize()
        s2 = ctx.ws_stats()
        for k in ("builds", "replans", "captures", "evictions"):
            assert s2[k] == s1[k], (name, k, s1, s2)
        assert torch.equal(L, L2), name
        for k, b in enumerate(order):
            T = STD[b][0]
            assert outs[k].shape == (80, T)
            assert torch.equal(outs[k], again[k]), (name, STD[b])
            assert torch.equal(outs[k], ref[b][0]), (name, STD[b], float((outs[k] - ref[b][0]).abs().max()))
            assert torch.equal(L[:, k], ref[b][1]), (name, STD[b])
            assert torch.equal(g0[k], ref[b][2]), (name, STD[b], float((g0[k] - ref[b][2]).abs().max()))
            assert float((outs[k] - vc[b]).abs().max()) <= 0.1 + 1e-6


def test_ragged_vc_pgd(full, std):
    """AVC_UPDATE_PGD passes through the ragged path: bitwise the single-utterance PGD attack (e2e, fp32)."""
    z, m, ctx = full
    src, vc, at, p0, te = std
    kw = dict(update="pgd", pgd_step=2e-3)
    outs, L, g0 = ctx.vc_attack_ragged("e2e", src, vc, te, p0, 0.1, 12, want_losses=True, want_grad0=True, **kw)
    for b in range(len(STD)):
        adv, Lr, gr = _single(ctx, "e2e", src, vc, p0, te, b, 12, **kw)
        assert torch.equal(outs[b], adv), (STD[b], float((outs[b] - adv).abs().max()))
        assert torch.equal(L[:, b], Lr) and torch.equal(g0[b], gr), STD[b]
        assert float((outs[b] - vc[b]).abs().max()) <= 0.1 + 1e-6


@pytest.mark.parametrize("kind", ["e2e", "fb"])
def test_ragged_vc_golden_T300(full, golden, kind):
    """The reference's own e2e / fb attacks at vc_src 280, vc_tgt 300, adv_tgt 260 frames (full_T300.npz), its two
    utterances inside one ragged batch with three other lengths: the bounds test_long_vc_golden_T300 holds the same
    kernels to."""
    z, m, ctx = full
    zl = golden("full_T300")
    osrc, ovc, oat, op0 = _utts([(129, 136), (77, 600), (33, 17)], 22)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    gs, gv, ga, gp = (dev(zl[k]) for k in ("vc_src", "vc_tgt", "adv_tgt", f"{kind}_ptb0"))
    # the golden utterances at positions 1 and 4 (the last block)
    src = [osrc[0], gs[0], osrc[1], osrc[2], gs[1]]
    vc = [ovc[0], gv[0], ovc[1], ovc[2], gv[1]]
    p0 = [op0[0], gp[0], op0[1], op0[2], gp[1]]
    at = [oat[0], ga[0], oat[1], oat[2], ga[1]]
    te = torch.cat([ctx.se_forward(a[None]) for a in at])
    outs, L, g0 = ctx.vc_attack_ragged(kind, src, vc, te, p0, 0.1, 10, want_losses=True, want_grad0=True)
    adv = torch.stack([outs[1], outs[4]]).cpu().numpy()
    check_adv(adv, zl[f"{kind}_adv_n10"], 10, kind=kind)
    g = torch.stack([g0[1], g0[4]]).cpu().numpy()
    assert rel(g, zl[f"{kind}_grad0"]) <= TOL_GRAD_REL_VC, rel(g, zl[f"{kind}_grad0"])
    np.testing.assert_allclose(L[:, [1, 4]].cpu().numpy().T, zl[f"{kind}_losses_n10"], rtol=2e-4, atol=1e-9)


@pytest.mark.parametrize("kind", ["e2e", "fb"])
def test_ragged_vc_grad0_vs_oracle(full, std, kind):
    """Iteration-0 gradients of the standard batch (fp32) vs the float64 oracle, per utterance, normwise: every
    utterance <= TOL_VC_GRAD_L2_MAX, the median <= 5 TOL_VC_GRAD_L2_MEDIAN (as test_long_vc_vs_oracle)."""
    z, m, ctx = full
    src, vc, at, p0, te = std
    w64 = oracle.Weights({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, dtype=np.float64)
    _, _, g0 = ctx.vc_attack_ragged(kind, src, vc, te, p0, 0.1, 1, want_grad0=True)
    e = []
    for b in range(len(STD)):
        rec = {}
        f64 = [t.cpu().double().numpy()[None] for t in (src[b], vc[b], at[b])]
        getattr(oracle, f"{kind}_attack")(w64, cfg_of(z), *f64, 0.1, 1, p0[b].cpu().double().numpy()[None], record=rec)
        gg = g0[b].cpu().numpy().astype(np.float64)
        e.append(float(np.linalg.norm(gg - rec["grad0"][0]) / np.linalg.norm(rec["grad0"][0])))
    print(f"ragged {kind} grad0 vs float64 oracle, per utterance {STD}: {e}")
    assert max(e) <= TOL_VC_GRAD_L2_MAX and float(np.median(e)) <= 5 * TOL_VC_GRAD_L2_MEDIAN, (kind, e)


def test_inference_ragged(full, std):
    """Each output equals m.inference of that utterance under the forced long engine bitwise, is within 1e-4 of
    the float64 oracle, and has 8 ceil(T_src / 8) frames."""
    z, m, ctx = full
    src, vc, at, p0, te = std
    w64 = oracle.Weights({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, dtype=np.float64)
    emb = torch.cat([ctx.se_forward(v[None]) for v in vc])
    for name, order in ORDERS.items():
        outs = ctx.inference_ragged(_pick(src, order), emb[order].contiguous())
        for k, b in enumerate(order):
            assert outs[k].shape == (80, _tn(STD[b][1])), (name, STD[b])
            ctx.set_engine("long")
            try:
                one = m.inference(src[b][None], vc[b][None])[0]
            finally:
                ctx.set_engine("auto")
            assert torch.equal(outs[k], one), (name, STD[b], float((outs[k] - one).abs().max()))
            if name == "shortest_last":
                ref = oracle.inference(w64, cfg_of(z), src[b].cpu().double().numpy()[None], vc[b].cpu().double().numpy()[None])
                assert rel(outs[k].cpu().numpy(), ref[0]) <= 1e-4, (STD[b], rel(outs[k].cpu().numpy(), ref[0]))


def test_attack_many_ragged(full):
    """12 utterances, max_batch 5, two workers on one GPU: results in input order; fp32 e2e and bf16 fb equal
    attack_utils.{e2e,fb}_attack on each utterance under the forced long engine bitwise; the emb kind equals
    attack_many(ragged=True)."""
    z, m, ctx = full
    pairs = [(64, 300), (300, 64), (128, 129), (77, 17), (450, 33), (33, 450), (129, 128), (200, 90), (96, 96),
             (128, 128), (600, 201), (90, 136)]
    src, vc, at, p0 = _utts(pairs, 23)
    res = {}
    for kind, prec in (("e2e", "fp32"), ("fb", "bf16")):
        res[kind] = batching.attack_many_ragged(kind, [m, m], vc, at, 0.1, 12, vc_srcs=src, ptb0s=p0, precision=prec,
                                                max_batch=5)
    ctx.set_engine("long")
    try:
        for kind, prec in (("e2e", "fp32"), ("fb", "bf16")):
            for i, (T, Ts) in enumerate(pairs):
                ref = FN[kind](m, src[i][None], vc[i][None], at[i][None], 0.1, 12, ptb0=p0[i][None],
                               precision=prec).detach()[0]
                assert res[kind][i].shape == (80, T)
                assert torch.equal(res[kind][i], ref), (kind, i, T, Ts, float((res[kind][i] - ref).abs().max()))
    finally:
        ctx.set_engine("auto")
    a = batching.attack_many_ragged("emb", [m, m], vc, at, 0.1, 12, ptb0s=p0, max_batch=5)
    b = batching.attack_many("emb", [m, m], vc, at, 0.1, 12, ptb0s=p0, max_batch=5, ragged=True)
    for i in range(len(pairs)):
        assert torch.equal(a[i], b[i]), i


def test_ragged_vc_refusals(full, std):
    z, m, ctx = full
    src, vc, at, p0, te = std
    ctx.set_engine("layered")
    try:
        with pytest.raises(RuntimeError, match="LAYERED"):
            ctx.vc_attack_ragged("e2e", src, vc, te, p0, 0.1, 2)
        with pytest.raises(RuntimeError, match="LAYERED"):
            ctx.inference_ragged(src, te)
    finally:
        ctx.set_engine("auto")
    with pytest.raises(RuntimeError, match="independent"):
        ctx.vc_attack_ragged("fb", src, vc, te, p0, 0.1, 2, reduction="mean")
    with pytest.raises(RuntimeError, match="source lengths for B="):
        ctx.vc_attack_ragged("e2e", src[:-1], vc, te, p0, 0.1, 2)
    short = src[:-1] + [src[-1][:, :16].contiguous()]
    with pytest.raises(RuntimeError, match="too short"):
        ctx.vc_attack_ragged("e2e", short, vc, te, p0, 0.1, 2)
    with pytest.raises(RuntimeError, match="too short"):
        ctx.inference_ragged(short, te)
    with pytest.raises(RuntimeError, match="ptb0 lengths"):
        ctx.vc_attack_ragged("e2e", src, vc, te, p0[:-1] + [p0[-1][:, :20].contiguous()], 0.1, 2)
    with pytest.raises(ValueError, match="emb attack only"):
        batching.attack_many("e2e", [m], vc, at, 0.1, 2, vc_srcs=src, ragged=True)


def test_ragged_vc_spectral_norm(golden):
    """sn=True Decoder: a ragged batch of one equals vc_attack under the forced long engine bitwise (fp32, n = 3:
    one power iteration per Decoder forward over the batch), and leaves the same u / v in the module."""
    z = golden("full_sn_T128")
    m0 = model_from_fixture(z)
    assert m0.decoder.sn
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    src, vc, at = (dev(z[k])[:1] for k in ("vc_src", "vc_tgt", "adv_tgt"))
    for kind in ("e2e", "fb"):
        p0 = dev(z[f"{kind}_ptb0"])[:1]
        m1, m2 = (copy.deepcopy(m0).to(DEV) for _ in range(2))
        c1, c2 = avc_native.vc_context_for(m1, DEV), avc_native.vc_context_for(m2, DEV)
        te = c1.se_forward(at)
        c1.set_engine("long")
        adv, L, g0 = c1.vc_attack(kind, src, vc, None, p0, 0.1, 3, want_losses=True, want_grad0=True, tgt_emb=te)
        outs, Lr, gr = c2.vc_attack_ragged(kind, [src[0]], [vc[0]], te, [p0[0]], 0.1, 3, want_losses=True,
                                           want_grad0=True)
        assert torch.equal(outs[0], adv[0]), (kind, float((outs[0] - adv[0]).abs().max()))
        assert torch.equal(Lr, L) and torch.equal(gr[0], g0[0]), kind
        moved = False
        for (k1, b1), (k2, b2) in zip(m1.decoder.state_dict().items(), m2.decoder.state_dict().items()):
            assert k1 == k2 and torch.equal(b1, b2), (kind, k1)
            if k1.endswith("weight_u"):
                moved |= not torch.equal(b1, m0.decoder.state_dict()[k1].to(DEV))
        assert moved, kind
