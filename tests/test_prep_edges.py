"""rgbnm_prep_weights / rgbnm_prep_weights_chain at the C ABI, whole buffers bit for bit (tests/prep_ref.py is the reference;
tests/test_prep_edges_cpu.py proves the reference, the comparison and the case lists).

The launch turns the fp32 masters into every operand shadow of both models, every step; until this file it was reached only
through model-level logit and gradient-norm bars.  Every launch here
- writes into guarded buffers (kernel_check.guarded: canary margins, checked bit-wise) whose bodies are pre-filled with a
  finite non-zero sentinel -- zeros only where the header says "left as the caller zeroed them" (`pair`, the ldn pad rows);
- reads a master with NaN in every alignment gap, before its first and after its last segment;
- is compared as WHOLE shadow / bias_perm / chain-image buffers on integer views with prep_ref.interpret: a stray write into
  a pad, a missing off-diagonal zero, a skipped shadow that was touched or a segment that was never written all differ;
  where the master holds NaN on purpose the output must be NaN (payload not compared);
- asserts prep_weights_kernel in the expected instantiation, once (torch.profiler).
The masters carry prep_ref.specials(): signed zeros, ties of both 16-bit types, fp16 subnormals down to half the smallest,
65504 / 65520 / 1e5, the bf16 overflow edge, fp32 subnormals, +-inf, NaN; add_identity diagonals carry identity_specials().

Found by this file: prep_weights_kernel formed every element as `w + (add_identity && r == c ? 1.0f : 0.0f)`, and -0.0f + 0.0f
is +0.0f: a master's -0 reached every shadow and chain image as +0 (all 43 launch tests failed on exactly those elements,
e.g. "small f32 ... shadow: 12 of 27408 elements differ, first [53]: got 0 (0x0) want -0 (0x80000000)").  The kernel now adds
1.0f on the diagonal only.

Run time on one MI355X: 44 tests, 6 s as a file of its own (2 s of it the first profiler start-up).
"""
import pytest
import torch

import prep_ref as P
import rgb_no_more_amd as rg
from kernel_check import guarded, launched
from prep_ref import BF16, F16, F32
from rgb_no_more_amd import chain, detfill, lib as L
from test_fp16_tuned_kernels import BF16_MARKS, F16_MARKS
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
F32_MARKS = ("<float>", "kernelIfE")


def instantiation(name):
    if any(m in name for m in BF16_MARKS):
        return BF16
    if any(m in name for m in F16_MARKS):
        return F16
    return F32 if any(m in name for m in F32_MARKS) else None


def expect_prep(names, T, where, alone=True):
    hits = [n for n in names if "prep_weights_kernel" in n]
    assert len(hits) == 1, f"{where}: {len(hits)} prep_weights_kernel launches; ran {sorted(set(names))}"
    assert instantiation(hits[0]) == T, f"{where}: wrong instantiation {hits[0]}"
    assert not alone or len(names) == 1, f"{where}: more than the one launch: {sorted(set(names))}"


def sentinel_buffer(n, T):
    g = guarded(n, None, T)
    P.fill_sentinel(g.t)
    return g


def run_launch(launch, T, *, bias=True, img_f=False, img_b=False, skip=0, entry="chain", given=None, where=""):
    """One launch over fresh guarded buffers (or over `given`, the buffers of an earlier launch), compared with the
    interpreter started from what the buffers held before.  Returns the buffers."""
    where = f"{where} {NAMES[T]} bias={int(bias)} img_f={int(img_f)} img_b={int(img_b)} skip={skip} entry={entry}"
    descs_dev = P.descs_to_device(launch.descs, DEV)
    if given is None:
        sh = guarded(launch.shadow_elems, None, T)
        launch.prefill(sh.t)
        bs = sentinel_buffer(launch.bias_elems, F32)
        fi = sentinel_buffer(launch.blocks * chain.BLOCK_ELEMS, BF16)
        bi = sentinel_buffer(launch.blocks * chain.BLOCK_ELEMS, BF16)
    else:
        sh, bs, fi, bi = given
    before = [g.t.clone() for g in (sh, bs, fi, bi)]
    lib = L.lib()

    def call():
        if entry == "plain":
            assert not (img_f or img_b or skip)
            return lib.rgbnm_prep_weights(L.dt_of(T), descs_dev.data_ptr(), len(launch.descs), launch.master.data_ptr(),
                                          sh.t.data_ptr(), bs.t.data_ptr() if bias else None, L.stream())
        return lib.rgbnm_prep_weights_chain(L.dt_of(T), descs_dev.data_ptr(), len(launch.descs), launch.master.data_ptr(),
                                            sh.t.data_ptr(), bs.t.data_ptr() if bias else None,
                                            fi.t.data_ptr() if img_f else None, bi.t.data_ptr() if img_b else None, skip,
                                            L.stream())
    rc, names = launched(call)
    L.check(rc, where)
    expect_prep(names, T, where)
    want = P.interpret(launch.descs, launch.master, T, before[0], before[1] if bias else None,
                       before[2] if img_f else None, before[3] if img_b else None, skip)
    for g, w, b, what in zip((sh, bs, fi, bi), want, before, ("shadow", "bias_perm", "chain_fwd", "chain_bwd")):
        g.check(f"{where} {what}", written=False)                      # the canary margins, bit-wise
        P.compare(g.t, b if w is None else w, f"{where} {what}")       # a buffer that was not handed over keeps its bits
    return sh, bs, fi, bi


@pytest.fixture(scope="module")
def launches():
    return {name: P.Launch(specs, 11 + i, DEV) for i, (name, specs) in enumerate({**P.SYNTH, **P.CHAIN}.items())}


@pytest.mark.parametrize("name", list(P.SYNTH))
@pytest.mark.parametrize("T", [F32, BF16, F16], ids=lambda t: NAMES[t])
def test_synthetic_descriptors(launches, T, name):
    """Tile-turn edges, ragged 32 x 32 tiles, ldn pads, pair, perm_heads, add_identity and the bias rules, per element type and
    through both entries; bias_perm = NULL leaves the bias buffer alone and writes the same shadows."""
    la = launches[name]
    run_launch(la, T, entry="plain", where=name)
    run_launch(la, T, bias=False, entry="chain", where=name)


@pytest.mark.parametrize("T", [F32, BF16, F16], ids=lambda t: NAMES[t])
def test_chain_kinds_without_images_are_plain_descriptors(launches, T):
    """chain_kind / chain_off are ignored when no image is given (the only form fp16 and fp32 accept)."""
    for name in P.CHAIN:
        run_launch(launches[name], T, entry="plain", where=name)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("img_f,img_b", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("name", list(P.CHAIN))
def test_chain_images(launches, name, img_f, img_b, skip):
    """Kinds 1 - 4 at depth 1 and 2 (chain_off), either or both images; skip_chain_shadows leaves the block Linears' shadows at
    the sentinel bit for bit while the other descriptors of the launch are written.  A second launch over the first one's
    output gives the same bits."""
    la = launches[name]
    bufs = run_launch(la, BF16, img_f=img_f, img_b=img_b, skip=skip, where=name)
    first = [g.t.clone() for g in bufs]
    run_launch(la, BF16, img_f=img_f, img_b=img_b, skip=skip, given=bufs, where=name + " again")
    for g, f, what in zip(bufs, first, ("shadow", "bias_perm", "chain_fwd", "chain_bwd")):
        P.compare(g.t, f, f"{name} second launch {what}")
    if skip:                                                       # (what interpret() was asked for, said once more in the open)
        sent = P.SENTINEL[2]
        for d in la.descs:
            if d.chain_kind:
                for off in (d.ws_off, d.wst_off):
                    seg = bufs[0].t[off:off + d.N * d.K].view(torch.int16)
                    assert bool((seg == sent).all()), f"{name}: skipped shadow of kind {d.chain_kind} was written"


# ----------------------------------------------------------------------------------------------------- the models' tables
def normalish_flat(n, seed):
    """detfill.normalish over n elements (a period of 1000003 values: no multiple of any tile or segment size)."""
    period = 1000003
    base = torch.from_numpy(detfill.normalish((min(n, period),), seed))
    return base.repeat(-(-n // period))[:n].contiguous() * 0.05


def fill_masters(m, descs, seed):
    """_flat <- normalish everywhere (alignment gaps too), the special values at the head of every Linear weight, in place."""
    flat = normalish_flat(m._flat.numel(), seed)
    for i, d in enumerate(descs):
        P.put_specials(flat[d.w_off:d.w_off + d.N * d.K].view(d.N, d.K), d.add_identity, shift=5 * i)
    m._flat.copy_(flat.to(DEV))


def reset_outputs(descs, *bufs):
    """Sentinel in every output buffer; zeros in the shadow segments the header leaves to the caller's zeroes (pair, ldn)."""
    for b in bufs:
        P.fill_sentinel(b)
    for d in descs:
        if d.pair or d.ldn > d.N:
            e_ws, e_wst = P.shadow_extent(d)
            bufs[0][d.ws_off:d.ws_off + e_ws] = 0
            bufs[0][d.wst_off:d.wst_off + e_wst] = 0


def vit(kind, **kw):
    args = dict(depth=1, n_classes=1000, emb=192, heads=3)
    args.update(kw)
    ver, sub = {"group": (1, True), "sep_sub": (2, True), "sep": (2, False), "concat": (3, True)}[kind]
    m = rg.ViT(3, 16, args["emb"], depth=args["depth"], n_classes=args["n_classes"], drop_p=0.0, device=DEV,
               num_heads=args["heads"], head_size=64, pixel_space="DCT", ver=ver, use_subblock=sub)
    assert m.embed_kind == kind
    return m


VITS = {"group-d2": lambda: vit("group", depth=2), "sep_sub": lambda: vit("sep_sub"), "sep": lambda: vit("sep"),
        "concat": lambda: vit("concat"), "classes10": lambda: vit("group", n_classes=10),
        "E384": lambda: vit("group", emb=384, heads=6)}


@pytest.mark.parametrize("tag", list(VITS))
def test_vit_descriptor_tables(tag):
    """ViT._flatten's table for every embed_kind, a padded class count (ldn) and a width that is not chain-eligible: the
    segments are pairwise disjoint, and _prep writes exactly what the interpreter says, in each dtype and prep mode."""
    m = VITS[tag]()
    m._ensure_flat()
    descs = P.descs_from_device(m._descs_dev)
    assert len(descs) == m._ndesc
    assert P.disjoint(P.desc_segments(descs)), tag
    eligible = m._chain_idx is not None
    assert eligible == (tag not in ("concat", "E384")), tag      # E = 192, 3 heads, 196 tokens
    assert any(d.ldn > d.N for d in descs) == (tag == "classes10")
    assert any(d.add_identity for d in descs) == (tag == "sep_sub")
    fill_masters(m, descs, 41)
    with torch.enable_grad():
        for T in (F32, BF16, F16):
            for mode in ({}, {"shadows": True}, {"chains": False}):
                if mode and not (eligible and T == BF16):
                    continue                                           # the modes differ only where images are written
                m._prep(T, **mode)                                     # (allocates the dtype's shadow buffer)
                imgs = eligible and T == BF16 and mode.get("chains", True)
                bufs = [m._shadow[T], m._bias_perm] + ([m._chain_img, m._chain_img_bwd] if eligible else [])
                reset_outputs(descs, *bufs)
                before = [b.clone() for b in bufs]
                _, names = launched(lambda: m._prep(T, **mode))
                where = f"ViT {tag} {NAMES[T]} {mode}"
                expect_prep(names, T, where, alone=False)
                skip = int(imgs and not mode.get("shadows", False))
                want = P.interpret(descs, m._flat, T, before[0], before[1], before[2] if imgs else None,
                                   before[3] if imgs else None, skip)
                for b, w, b0, what in zip(bufs, want, before, ("shadow", "bias_perm", "chain_fwd", "chain_bwd")):
                    P.compare(b, b0 if w is None else w, f"{where} {what}")


def test_swin_descriptor_table():
    """SwinTransformerV2._flatten's table at SwinV2-T's widths (depth 2 per stage): pair (stage 1), bias_mode 1 and 2."""
    m = rg.SwinTransformerV2(img_size=256, patch_size=4, embed_dim=96, depths=[2, 2, 2, 2], num_heads=[3, 6, 12, 24],
                             window_size=8, mlp_ratio=4.0, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, qkv_bias=True,
                             ape=False, patch_norm=True, pretrained_window_sizes=[0] * 4, device=DEV, pixel_space="dct")
    m._ensure_flat()
    descs = P.descs_from_device(m._descs_dev)
    assert len(descs) == m._ndesc
    assert P.disjoint(P.desc_segments(descs))
    assert {(d.pair, d.bias_mode) for d in descs} >= {(1, 1), (1, 2), (0, 1), (0, 2)}
    fill_masters(m, descs, 43)
    for T in (F32, BF16, F16):
        m._prep(T)
        bufs = [m._shadow[T], m._bias_prep]
        reset_outputs(descs, *bufs)
        before = [b.clone() for b in bufs]
        _, names = launched(lambda: m._prep(T))
        where = f"SwinV2-T {NAMES[T]}"
        expect_prep(names, T, where, alone=False)
        want = P.interpret(descs, m._flat, T, before[0], before[1])
        for b, w, what in zip(bufs, want, ("shadow", "bias_prep")):
            P.compare(b, w, f"{where} {what}")


def test_tile_regimes_of_the_models_tables_are_in_the_synthetic_list():
    """Every tile-loop regime a model descriptor sits in is one the synthetic cases walk (prep_ref.tile_regime)."""
    walked = {P.tile_regime(s["N"], s["K"]) for specs in P.SYNTH.values() for s in specs}
    m = vit("group", n_classes=10)
    m._ensure_flat()
    got = {P.tile_regime(d.N, d.K) for d in P.descs_from_device(m._descs_dev)}
    assert got <= walked, got - walked
    assert walked >= {"1", "64", "65", "128", "129", ">256"}
