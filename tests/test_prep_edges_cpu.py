"""CPU companion of tests/test_prep_edges.py: the reference interpreter (tests/prep_ref.py) against plain torch, the comparison
function against seeded defects, the case lists against the kernel's tile loop, and the refusals of the two entries."""
import einops
import pytest
import torch

import prep_ref as P
from prep_ref import BF16, F16, F32
from rgb_no_more_amd import chain, lib as L

EINVAL = -1
TYPES = [F32, BF16, F16]


def fresh(launch, T):
    sh = launch.prefill(torch.empty(launch.shadow_elems, dtype=T))
    bs = P.fill_sentinel(torch.empty(launch.bias_elems, dtype=F32))
    return sh, bs


# --------------------------------------------------------------------------------------------------------- the interpreter
@pytest.mark.parametrize("T", TYPES)
def test_interpreter_against_plain_torch(T):
    """W.to(T), .t(), torch.block_diag and an einops rearrangement, one descriptor at a time, with everything else untouched."""
    g = torch.Generator().manual_seed(5)
    sent = torch.tensor(P.SENTINEL[torch.tensor([], dtype=T).element_size()]).to(P.INT[torch.tensor([], dtype=T).element_size()])

    def run(d, master, zero=False):
        e_ws, e_wst = P.shadow_extent(d)
        d.ws_off, d.wst_off, d.bperm_off = 16, 16 + e_ws + 24, 8
        sh = P.fill_sentinel(torch.empty(d.wst_off + e_wst + 16, dtype=T))
        if zero:
            sh[16:16 + e_ws] = 0
            sh[d.wst_off:d.wst_off + e_wst] = 0
        bs = P.fill_sentinel(torch.empty(4096, dtype=F32))
        out, bias, _, _ = P.interpret([d], master, T, sh, bs)
        it = P.INT[sh.element_size()]
        for pad in (out[:16], out[16 + e_ws:d.wst_off], out[d.wst_off + e_wst:]):
            assert bool((pad.view(it) == sent).all())
        assert bool((bias[:8].view(torch.int32) == P.SENTINEL[4]).all())
        return out[16:16 + e_ws], out[d.wst_off:d.wst_off + e_wst], bias[8:]

    def same(a, b):
        P.compare(a.contiguous().view(-1), b.contiguous().view(-1), "anchor")

    # plain, with a bias
    W, b = torch.randn(33, 31, generator=g), torch.randn(33, generator=g)
    master = torch.cat([W.reshape(-1), b])
    ws, wst, bias = run(P.desc(33, 31, w_off=0, b_off=33 * 31, bias_mode=1), master)
    same(ws.view(33, 31), W.to(T))
    same(wst.view(31, 33), W.to(T).t())
    same(bias[:33], b)
    assert bool((bias[33:].view(torch.int32) == P.SENTINEL[4]).all())
    # ldn: the transposed shadow has pitch 16, pad columns and rows untouched
    W = torch.randn(10, 24, generator=g)
    ws, wst, _ = run(P.desc(10, 24, ldn=16), W.reshape(-1))
    same(ws[:240].view(10, 24), W.to(T))
    assert bool((ws[240:].view(P.INT[ws.element_size()]) == sent).all())
    same(wst.view(24, 16)[:, :10], W.to(T).t())
    assert bool((wst.view(24, 16)[:, 10:].contiguous().view(P.INT[ws.element_size()]) == sent).all())
    # pair over zeroed segments: torch.block_diag
    W, b = torch.randn(12, 20, generator=g), torch.randn(12, generator=g)
    ws, wst, bias = run(P.desc(12, 20, pair=1, w_off=0, b_off=240, bias_mode=1), torch.cat([W.reshape(-1), b]), zero=True)
    same(ws.view(24, 40), torch.block_diag(W, W).to(T))
    same(wst.view(40, 24), torch.block_diag(W.t(), W.t()).to(T))
    same(bias[:24], torch.cat([b, b]))
    # bias_mode 2: q | 0 | v
    W, q, v = torch.randn(12, 8, generator=g), torch.randn(4, generator=g), torch.randn(4, generator=g)
    _, _, bias = run(P.desc(12, 8, w_off=0, b_off=96, b2_off=100, bias_mode=2), torch.cat([W.reshape(-1), q, v]))
    same(bias[:12], torch.cat([q, torch.zeros(4), v]))
    # perm_heads: the header's '(h d qkv)' split, written with einops; add_identity on the SHADOW's diagonal, in fp32
    for heads in (3, 6):
        N, K = heads * 192, 64 * heads
        W, b = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        P.put_specials(W, 1)
        master = torch.cat([W.reshape(-1), b])
        ws, wst, bias = run(P.desc(N, K, w_off=0, b_off=N * K, perm_heads=heads, add_identity=1), master)
        V = einops.rearrange(W, "(h d qkv) k -> (qkv h d) k", h=heads, d=64, qkv=3)
        V = V.clone()
        V.diagonal().add_(1.0)                                       # fp32 + fp32: rounds before the cast; ONLY the diagonal
        same(ws.view(N, K), V.to(T))
        same(wst.view(K, N), V.to(T).t())
        same(bias[:N], einops.rearrange(b, "(h d qkv) -> (qkv h d)", h=heads, d=64, qkv=3))


def test_chain_images_gather_the_reference_shadow():
    """The images are chain.block_index / block_index_bwd over the reference's own unskipped shadow, block by block."""
    la = P.Launch(P.CHAIN["depth2"], 3)
    sh, bs = fresh(la, BF16)
    img = P.fill_sentinel(torch.empty(2 * chain.BLOCK_ELEMS, dtype=BF16))
    full, _, _, _ = P.interpret(la.descs, la.master, BF16, sh, bs)
    for skip in (0, 1):
        out, _, fi, bi = P.interpret(la.descs, la.master, BF16, sh, bs, img, img, skip)
        for blk in range(2):
            d = {x.chain_kind: x for x in la.descs if x.chain_kind and x.chain_off == blk * chain.BLOCK_ELEMS}
            idx = torch.from_numpy(chain.block_index(*(d[k].ws_off for k in (1, 2, 3, 4))))
            idb = torch.from_numpy(chain.block_index_bwd(*(d[k].wst_off for k in (1, 2, 3, 4))))
            P.compare(fi[blk * chain.BLOCK_ELEMS:(blk + 1) * chain.BLOCK_ELEMS], full[idx], f"fwd image, block {blk}")
            P.compare(bi[blk * chain.BLOCK_ELEMS:(blk + 1) * chain.BLOCK_ELEMS], full[idb], f"bwd image, block {blk}")
        if skip:
            for x in la.descs:
                seg = out[x.ws_off:x.ws_off + x.N * x.K].view(torch.int16)
                assert bool((seg == P.SENTINEL[2]).all()) == bool(x.chain_kind)
        else:
            P.compare(out, full, "unskipped shadows")


# --------------------------------------------------------------------------------------------------------- seeded defects
def rtz(x, T):
    """fp32 -> T rounded toward zero."""
    if T == F32:
        return x.clone()
    if T == BF16:
        return (x.view(torch.int32) & -65536).view(F32).to(BF16)            # (NaN payloads live in the high half here)
    h = x.to(F16)
    away = (h.float().abs() > x.abs()) & ~torch.isnan(x)
    return torch.where(away, (h.view(torch.int16) - 1).view(F16), h)


def ftz16(x, T):
    h = x.to(T)
    if T != F16:
        return h
    sub = (h.float().abs() < 2.0 ** -14) & (h != 0)
    return torch.where(sub, torch.copysign(torch.zeros_like(h), h), h)


def kernel_like(launch, T, shadow, bias, defect=None):
    """What prep_weights_kernel stores, written from its index arithmetic (one flat scatter per store statement), with one
    seeded defect.  Not the reference: the thing the reference and prep_ref.compare have to tell apart."""
    shadow, bias = shadow.clone(), bias.clone()
    m = launch.master
    for d in launch.descs:
        N, K = d.N, d.K
        r = torch.arange(N).view(N, 1).expand(N, K)
        c = torch.arange(K).view(1, K).expand(N, K)
        src = r
        if d.perm_heads > 0:
            inner = d.perm_heads * 64
            src = ((r % inner) // 64) * 192 + (r % 64) * 3 + r // inner
        v = m[d.w_off + src * K + c]
        if d.add_identity:
            diag = (src == c) if defect == "identity_on_source_row" else (r == c)
            # `v + (diag ? 1.0f : 0.0f)` is not the same thing: -0.0f + 0.0f is +0.0f off the diagonal
            v = v + diag.to(F32) if defect == "identity_adds_zero_elsewhere" else torch.where(diag, v + 1.0, v)
        cast = {"round_toward_zero": rtz, "fp16_subnormals_flushed": ftz16}.get(defect, lambda x, t: x.to(t))
        o = cast(v.contiguous(), T)
        if d.pair:
            shadow[d.ws_off + r * 2 * K + c] = o
            shadow[d.ws_off + (N + r) * 2 * K + (0 if defect == "pair_second_copy_at_N_0" else K) + c] = o
            shadow[d.wst_off + c * 2 * N + r] = o
            shadow[d.wst_off + (K + c) * 2 * N + N + r] = o
        else:
            shadow[d.ws_off + r * K + c] = o
            ld = N if defect == "transposed_pitch_N" or d.ldn <= 0 else d.ldn
            shadow[d.wst_off + c * ld + r] = o
        i = torch.arange(N)
        if d.perm_heads > 0:
            inner = d.perm_heads * 64
            bias[d.bperm_off + i] = m[d.b_off + ((i % inner) // 64) * 192 + (i % 64) * 3 + i // inner]
        elif d.bias_mode:
            third = N // 3
            if d.bias_mode == 1:
                b = m[d.b_off + i]
            elif defect == "v_bias_at_a_third":
                b = torch.where(i < third, m[d.b_off + i.clamp(max=third - 1)],
                                torch.where(i < 2 * third, m[d.b2_off + (i - third).clamp(0, third - 1)], torch.zeros(())))
            else:
                b = torch.where(i < third, m[d.b_off + i.clamp(max=third - 1)],
                                torch.where(i < 2 * third, torch.zeros(()), m[d.b2_off + (i - 2 * third).clamp(min=0)]))
            bias[d.bperm_off + i] = b
            if d.pair:
                bias[d.bperm_off + N + i] = b
    return shadow, bias


def passes(launch, T, defect):
    sh, bs = fresh(launch, T)
    want_s, want_b, _, _ = P.interpret(launch.descs, launch.master, T, sh, bs)
    got_s, got_b = kernel_like(launch, T, sh, bs, defect)
    try:
        P.compare(got_s, want_s, "shadow")
        P.compare(got_b, want_b, "bias_perm")
    except AssertionError:
        return False
    return True


CPU_LAUNCHES = ("small", "ldn", "pair", "identity", "bias")          # (the others only add size)


@pytest.fixture(scope="module")
def launches():
    return {name: P.Launch(P.SYNTH[name], 11 + i) for i, name in enumerate(P.SYNTH) if name in CPU_LAUNCHES}


@pytest.mark.parametrize("T", TYPES)
def test_a_faithful_copy_of_what_the_kernel_writes_passes(launches, T):
    for name, la in launches.items():
        assert passes(la, T, None), name


# defect -> (launch that must expose it, the element types in which it differs)
DEFECTS = {"pair_second_copy_at_N_0": ("pair", TYPES), "identity_on_source_row": ("identity", TYPES),
           "identity_adds_zero_elsewhere": ("identity", TYPES),
           "v_bias_at_a_third": ("bias", TYPES), "transposed_pitch_N": ("ldn", TYPES),
           "round_toward_zero": ("small", [BF16, F16]), "fp16_subnormals_flushed": ("small", [F16])}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_seeded_defects_are_rejected(launches, defect):
    name, types = DEFECTS[defect]
    for T in types:
        assert not passes(launches[name], T, defect), (defect, name, T)


def test_each_special_value_earns_its_place():
    """Per 16-bit type the specials hold a tie, a value that overflows and (fp16) subnormal results, and both casts keep NaN."""
    sp = P.specials()
    for T in (BF16, F16):
        assert bool((rtz(sp, T).float() != sp.to(T).float())[~torch.isnan(sp)].any())
        assert bool(torch.isinf(sp.to(T))[torch.isfinite(sp)].any())
        assert bool(torch.isnan(sp.to(T)).any())
    h = sp.to(F16).float().abs()
    assert bool(((h > 0) & (h < 2.0 ** -14)).any()) and float(h[h > 0].min()) == 2.0 ** -24
    assert bool(((sp.abs() == 2.0 ** -25) & (sp.to(F16) == 0)).any())             # half the smallest subnormal: tie to even, zero
    ids = P.identity_specials()
    one = torch.ones(())
    for T in (BF16, F16):
        x = ids.double() + 1.0                                                    # the sum NOT rounded to fp32 first ...
        in12 = (x >= 1) & (x < 2)
        p = 7 if T == BF16 else 10
        once = torch.round(x[in12] * 2.0 ** p) / 2.0 ** p                         # ... and rounded to T once (half to even)
        assert bool(((ids + one).to(T)[in12].double() != once).any()), T
        after = (ids.to(T).float() + one).to(T)                                   # the identity added after the cast
        fin = torch.isfinite(ids)
        assert bool(((ids + one).to(T)[fin] != after[fin]).any()), T


# --------------------------------------------------------------------------------------------------------- the case lists
def test_case_lists_hold_what_the_issue_lists():
    shapes = {(s["N"], s["K"]) for specs in P.SYNTH.values() for s in specs}
    assert shapes >= {(1, 8), (8, 8), (31, 33), (32, 32), (33, 31), (40, 200), (256, 256), (264, 256), (512, 256), (520, 256),
                      (1000, 192)}
    every = [s for specs in P.SYNTH.values() for s in specs]
    assert {(s["N"], s["ldn"]) for s in every if s["ldn"]} >= {(1000, 1000), (1000, 1008), (10, 16)}
    assert all(s["zero_pad"] for s in every if (s["N"], s["ldn"]) == (10, 16))
    assert {(s["N"], s["K"]) for s in every if s["pair"]} >= {(96, 96), (288, 96), (96, 384)}
    assert {(s["perm_heads"], s["K"]) for s in every if s["perm_heads"]} >= {(3, 192), (6, 384), (12, 768)}
    assert {(s["N"], s["K"]) for s in every if s["add_identity"]} >= {(192, 192), (192, 384)}
    assert {(s["bias_mode"], s["pair"]) for s in every} >= {(m, p) for m in (0, 1, 2) for p in (0, 1)}
    for name, specs in P.CHAIN.items():
        kinds = sorted((s["block"], s["chain_kind"]) for s in specs if s["chain_kind"])
        depth = 1 + max(b for b, _ in kinds)
        assert kinds == [(b, k) for b in range(depth) for k in (1, 2, 3, 4)], name
        assert any(not s["chain_kind"] for s in specs), name                     # an unskipped descriptor in the same launch
    assert {1 + max(s["block"] for s in specs) for specs in P.CHAIN.values()} == {1, 2}


def test_synthetic_segments_are_adjacent_and_disjoint():
    for name, specs in {**P.SYNTH, **P.CHAIN}.items():
        la = P.Launch(specs, 1, with_specials=False)
        assert P.disjoint(la.segs), name
        assert P.disjoint(P.desc_segments(la.descs)), name
        sh = sorted((o, o + n) for b, o, n, _ in la.segs if b == "shadow")
        assert all(0 <= b0 - a1 < 8 for (_, a1), (b0, _) in zip(sh, sh[1:])), name
        nan = torch.isnan(la.master)
        covered = torch.zeros_like(nan)
        for b, o, n, _ in la.segs:
            if b == "master":
                covered[o:o + n] = True
        assert bool((nan == ~covered).all()), name                               # NaN in every gap, before and after
        assert bool(nan[:8].all()) and bool(nan[-64:].all())
    assert not P.disjoint([("shadow", 0, 10, 0), ("shadow", 9, 4, 1)])


def test_tile_loop_copy_and_the_edges_the_cases_reach():
    """64 workgroups, two tiles per turn: the cases sit on 1, 64, 65, 128, 129 and more than 256 tiles per descriptor."""
    assert P.tile_turns(1, 8) == (1, 1, [(1, 0)])
    assert P.tile_turns(256, 256) == (64, 1, [(64, 0)])
    assert P.tile_turns(264, 256) == (72, 1, [(64, 8)])
    assert P.tile_turns(160, 416) == (65, 1, [(64, 1)])
    assert P.tile_turns(512, 256) == (128, 1, [(64, 64)])
    assert P.tile_turns(96, 1376) == (129, 2, [(64, 64), (1, 0)])
    assert P.tile_turns(520, 256) == (136, 2, [(64, 64), (8, 0)])
    assert P.tile_turns(1000, 192) == (192, 2, [(64, 64), (64, 0)])
    assert P.tile_turns(2304, 768)[:2] == (1728, 14)
    reached = {P.tile_regime(s["N"], s["K"]) for specs in P.SYNTH.values() for s in specs}
    assert reached >= {"1", "<64", "64", "65", "65..127", "128", "129", "129..256", ">256"}, reached
    ragged = [(s["N"] % 32 != 0, s["K"] % 32 != 0) for specs in P.SYNTH.values() for s in specs]
    assert set(ragged) == {(False, False), (False, True), (True, False), (True, True)}


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_before_any_device_call():
    """Pointers that are never followed: every refusal returns before a launch."""
    lib = L.lib()
    ok = dict(dtype=L.DT_BF16, descs=0x1000, ndesc=4, master=0x2000, shadow=0x3000, bias=0x4000, img_f=None, img_b=None, skip=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.rgbnm_prep_weights_chain(a["dtype"], a["descs"], a["ndesc"], a["master"], a["shadow"], a["bias"], a["img_f"],
                                            a["img_b"], a["skip"], None)
    for dt in (L.DT_F16, L.DT_F32):
        for imgs in (dict(img_f=0x5000), dict(img_b=0x6000), dict(img_f=0x5000, img_b=0x6000)):
            assert call(dtype=dt, **imgs) == EINVAL, (dt, imgs)
    for dt in (L.DT_BF16, L.DT_F16, L.DT_F32):
        assert call(dtype=dt, skip=1) == EINVAL, dt
    for n in (0, -1):
        assert call(ndesc=n) == EINVAL, n
    for k in ("master", "shadow", "descs"):
        assert call(**{k: None}) == EINVAL, k
    for dt in (3, -1, 99):
        assert call(dtype=dt) == EINVAL, dt
        assert lib.rgbnm_prep_weights(dt, 0x1000, 4, 0x2000, 0x3000, 0x4000, None) == EINVAL, dt
    assert lib.rgbnm_prep_weights(L.DT_F32, None, 4, 0x2000, 0x3000, 0x4000, None) == EINVAL
    assert lib.rgbnm_prep_weights(L.DT_F32, 0x1000, 0, 0x2000, 0x3000, 0x4000, None) == EINVAL
    assert lib.rgbnm_prep_weights(L.DT_F32, 0x1000, 4, None, 0x3000, 0x4000, None) == EINVAL
    assert lib.rgbnm_prep_weights(L.DT_F32, 0x1000, 4, 0x2000, None, 0x4000, None) == EINVAL
