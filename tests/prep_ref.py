"""Reference of rgbnm_prep_weights / rgbnm_prep_weights_chain (include/rgbnm.h: rgbnm_linear_desc): a plain torch interpreter
of a list of lib.LinearDesc, the special values the tests put into the masters, the bit-wise comparison both test files use
and a Python copy of the kernel's tile loop.  A plain module, imported by name (tests/test_prep_edges.py, _cpu.py).

interpret(descs, master, T, shadow, bias, img_f, img_b, skip) returns the expected WHOLE shadow buffer, bias_perm buffer and
chain images, starting from clones of what the caller had in them: everything a descriptor does not write keeps the caller's
bits.  Per descriptor (N, K; W = master[w_off ..] as [N, K]):
- V[r, c] = W[src(r), c], src the '(h d qkv)' de-interleave of the header when perm_heads > 0 (shadow row
  s3 * heads * 64 + h * 64 + d  <-  master row h * 192 + d * 3 + s3), else r;  add_identity: V[r, r] += 1.0f IN FP32;
- [N, K] shadow at ws_off = V.to(T) (torch's cast: round to nearest even, subnormals kept, overflow to inf);
- [K, N] shadow at wst_off = the same values transposed, row pitch ldn or N;
- pair: both shadows are diag(V, V), [2N, 2K] with pitch 2K and [2K, 2N] with pitch 2N; only the diagonal blocks are written;
- bias_perm (if given): perm_heads > 0: master[b_off + src(i)];  bias_mode 1: master[b_off + i];  bias_mode 2: q | 0 | v with
  q = master[b_off ..] and v = master[b2_off ..], N / 3 each;  the bias_mode rules write the N values twice under `pair`;
- chain images (bf16, if given; chain_kind is ignored when neither is): rgb-no-more_amd/chain.py's block_index /
  block_index_bwd gather over the REFERENCE shadow -- never the kernel's --, the block's image at chain_off;
- skip != 0: descriptors with a chain_kind leave both shadows alone (their bias is still written).
"""
import ctypes as C

import numpy as np
import torch

from rgb_no_more_amd import chain
from rgb_no_more_amd import lib as L

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
INT = {2: torch.int16, 4: torch.int32}
# what the outputs hold before a launch where a case does not test "left as zeroed": finite, non-zero, the same bits in
# every element (so that a stray write of ANY weight value shows), never a value the masters hold
SENTINEL = {2: 0x3C5A, 4: 0x3F5A5A5A}


def desc(N, K, w_off=0, b_off=0, ws_off=0, wst_off=0, bperm_off=0, perm_heads=0, add_identity=0, ldn=0, pair=0, chain_kind=0,
         chain_off=0, bias_mode=0, b2_off=0):
    return L.LinearDesc(w_off, b_off, ws_off, wst_off, bperm_off, N, K, perm_heads, add_identity, ldn, pair, chain_kind,
                        chain_off, bias_mode, 0, b2_off)


def descs_array(descs):
    arr = (L.LinearDesc * len(descs))()
    for i, d in enumerate(descs):
        arr[i] = d
    return arr


def descs_to_device(descs, device):
    return torch.frombuffer(bytearray(bytes(descs_array(descs))), dtype=torch.uint8).to(device)


def descs_from_device(t):
    """The model's own table (a uint8 device tensor, e.g. ViT._descs_dev) back as a list of lib.LinearDesc."""
    raw = bytes(t.cpu().numpy().tobytes())
    n = len(raw) // C.sizeof(L.LinearDesc)
    assert n * C.sizeof(L.LinearDesc) == len(raw)
    return [L.LinearDesc.from_buffer_copy(raw[i * C.sizeof(L.LinearDesc):(i + 1) * C.sizeof(L.LinearDesc)]) for i in range(n)]


def qkv_src_rows(N, heads):
    """Master row of every shadow row: the header's 'b n (h d qkv) -> (qkv) b h n d' split, 64 dims per head."""
    assert N == heads * 64 * 3
    return torch.arange(N).view(heads, 64, 3).permute(2, 0, 1).reshape(-1)


_KIND_TABLES = {}


def _kind_tables():
    """Per image position of one block: (kind 1..4, element offset inside that Linear's shadow), forward and backward, taken
    from chain.block_index / block_index_bwd by giving every Linear a base of its own."""
    if not _KIND_TABLES:
        span = 1 << 40
        for name, fn in (("f", chain.block_index), ("b", chain.block_index_bwd)):
            idx = fn(1 * span, 2 * span, 3 * span, 4 * span)
            _KIND_TABLES[name] = (torch.from_numpy(idx // span), torch.from_numpy(idx % span))
    return _KIND_TABLES


def shadow_extent(d):
    """(elements of the [N, K] segment, elements of the [K, N] segment) a descriptor may touch, pads included."""
    if d.pair:
        return 4 * d.N * d.K, 4 * d.N * d.K
    ld = d.ldn if d.ldn > 0 else d.N
    return ld * d.K, d.K * ld


def interpret(descs, master, T, shadow, bias=None, img_f=None, img_b=None, skip=0):
    """-> (shadow, bias, img_f, img_b) expected after the launch; inputs are not modified.  All tensors on one device."""
    dev = master.device
    shadow = shadow.clone()
    bias = None if bias is None else bias.clone()
    img_f = None if img_f is None else img_f.clone()
    img_b = None if img_b is None else img_b.clone()
    images = img_f is not None or img_b is not None
    assert not images or T == BF16
    assert not skip or images
    full = None
    if images:
        # the chain images gather from a shadow in which NOTHING is skipped
        full = torch.zeros_like(shadow)
    for d in descs:
        N, K = d.N, d.K
        assert not (d.perm_heads > 0 and d.pair), "no caller pairs a qkv-permuted Linear"
        src = qkv_src_rows(N, d.perm_heads).to(dev) if d.perm_heads > 0 else None
        V = master[d.w_off:d.w_off + N * K].view(N, K)
        if src is not None:
            V = V[src]
        if d.add_identity:
            V = V.clone()
            i = torch.arange(min(N, K), device=dev)
            V[i, i] = V[i, i] + torch.ones((), dtype=F32, device=dev)
        Vc = V.to(T)
        kind = d.chain_kind if images else 0
        targets = [full] if kind else []
        if not (kind and skip):
            targets.append(shadow)
        for buf in targets:
            if d.pair:
                a = buf[d.ws_off:d.ws_off + 4 * N * K].view(2 * N, 2 * K)
                a[:N, :K] = Vc
                a[N:, K:] = Vc
                b = buf[d.wst_off:d.wst_off + 4 * N * K].view(2 * K, 2 * N)
                b[:K, :N] = Vc.t()
                b[K:, N:] = Vc.t()
            else:
                buf[d.ws_off:d.ws_off + N * K].view(N, K).copy_(Vc)
                ld = d.ldn if d.ldn > 0 else N
                torch.as_strided(buf, (K, N), (ld, 1), d.wst_off).copy_(Vc.t())
        if bias is not None:
            v = None
            if d.perm_heads > 0:
                v = master[d.b_off:d.b_off + N][src]
            elif d.bias_mode == 1:
                v = master[d.b_off:d.b_off + N]
            elif d.bias_mode:
                third = N // 3
                v = torch.zeros(N, dtype=F32, device=dev)
                v[:third] = master[d.b_off:d.b_off + third]
                v[2 * third:] = master[d.b2_off:d.b2_off + N - 2 * third]
            if v is not None:
                bias[d.bperm_off:d.bperm_off + N] = v
                if d.pair and d.perm_heads <= 0:
                    bias[d.bperm_off + N:d.bperm_off + 2 * N] = v
        if kind:
            tabs = _kind_tables()
            for img, which, base in ((img_f, "f", d.ws_off), (img_b, "b", d.wst_off)):
                if img is None:
                    continue
                kinds, rel = tabs[which]
                pos = (kinds == kind).nonzero().flatten()
                img[d.chain_off + pos.to(dev)] = full[(base + rel[pos]).to(dev)]
    return shadow, bias, img_f, img_b


def compare(got, want, where):
    """Whole-buffer, bit for bit (integer views).  Where `want` is NaN -- only a NaN of the master gets there: the sentinel is
    finite -- `got` must be NaN, its payload is not compared.  Raises AssertionError naming the first differences."""
    assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape, got.dtype, want.dtype)
    it = INT[got.element_size()]
    gb, wb = got.contiguous().view(it), want.contiguous().view(it)
    nan = torch.isnan(want)
    bad = torch.where(nan, ~torch.isnan(got), gb != wb)
    n = int(bad.sum())
    if n:
        idx = bad.nonzero().flatten()[:6]
        mask = (1 << (8 * got.element_size())) - 1
        msg = "; ".join(f"[{int(i)}]: got {float(got[i]):.9g} (0x{int(gb[i]) & mask:x}) want {float(want[i]):.9g} "
                        f"(0x{int(wb[i]) & mask:x})" for i in idx)
        raise AssertionError(f"{where}: {n} of {got.numel()} elements differ, first {msg}")


def fill_sentinel(t):
    t.view(INT[t.element_size()]).fill_(SENTINEL[t.element_size()])
    return t


# ----------------------------------------------------------------------------------------------------- special values
def specials():
    """fp32 values at which a cast goes wrong first: signed zeros, ties between neighbours of bf16 and of fp16 (both parities,
    and one fp32 ulp to either side), the fp16 subnormal range down to half the smallest subnormal, the fp16 overflow edge,
    the bf16 one, fp32 subnormals (bf16 keeps them), infinities and NaN."""
    e = 2.0 ** -23
    v = [0.0, -0.0]
    for h in (2.0 ** -8, 2.0 ** -11):                        # half an ulp of bf16 / fp16 at 1.0
        v += [1 + h, 1 + 3 * h, 1 + h + e, 1 + h - e, 1 + 3 * h + e, 1 + 3 * h - e, -(1 + h), -(1 + 3 * h)]
    s = 2.0 ** -24                                           # smallest fp16 subnormal
    v += [s, s / 2, s / 2 * (1 + e), s / 2 * (1 - e / 2), 1.5 * s, 1.5 * s * (1 + e), 2.5 * s, 1023 * s, 1023.5 * s, 2.0 ** -14,
          2.0 ** -14 - s / 2, -s, -s / 2, -1.5 * s, s / 4]
    v += [65504.0, 65519.996, 65520.0, 65536.0, 1e5, -65520.0, -1e5]
    big = float(np.finfo(np.float32).max)
    v += [big, -big, (2 - 2.0 ** -7) * 2.0 ** 127, (2 - 2.0 ** -8) * 2.0 ** 127]      # bf16 max, and the tie between it and 2^128
    v += [1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * (1 + e), 2.0 ** -149, 2.0 ** -126]
    v += [float("inf"), float("-inf"), float("nan")]
    return torch.tensor(v, dtype=torch.float64).to(F32)


def identity_specials():
    """Diagonal values of an add_identity weight whose fp32 sum with 1.0 rounds BEFORE the cast: adding the identity after
    the cast, or in higher precision, gives other bits."""
    v = [2.0 ** -25, -2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -8 + 2.0 ** -25, 2.0 ** -11 + 2.0 ** -25,
         2.0 ** -8 - 2.0 ** -26, -1.0, -1.0 + 2.0 ** -24, 65503.0, 65519.0, float("inf"), float("-inf"), float("nan"), -0.0]
    return torch.tensor(v, dtype=torch.float64).to(F32)


def put_specials(W, add_identity, shift=0):
    """Overwrite the head of W [N, K] (row-major) with the special values, cycled from `shift` on so that the small cases share
    the list between them; an add_identity weight also gets identity_specials on its leading diagonal.  In place."""
    N, K = W.shape
    sp = specials().to(W.device)
    n = min(sp.numel(), N * K)
    W.view(-1)[:n] = sp.roll(-shift)[:n]
    if add_identity:
        ids = identity_specials().to(W.device)
        m = min(ids.numel(), min(N, K))
        i = torch.arange(m, device=W.device) + (min(N, K) - m)      # the END of the diagonal: the head holds the specials
        W[i, i] = ids[:m]
    return W


# ----------------------------------------------------------------------------------------------------- the tile loop
WGS, TU, TILE = 64, 2, 32


def tile_turns(N, K):
    """Python copy of prep_weights_kernel's tile loop (64 workgroups per descriptor, two 32 x 32 tiles per workgroup and turn:
    `for (t0 = blockIdx.x; t0 < tiles; t0 += TU * gridDim.x)`, tile u of a turn is t0 + u * gridDim.x).
    -> (tiles, turns of the busiest workgroup, [per turn: (workgroups whose slot 0 holds a tile, ... slot 1)])."""
    tiles = -(-N // TILE) * -(-K // TILE)
    per_turn = {}
    seen = []
    for wg in range(WGS):
        turn = 0
        t0 = wg
        while t0 < tiles:
            for u in range(TU):
                t = t0 + u * WGS
                if t < tiles:
                    seen.append(t)
                    per_turn.setdefault(turn, [0] * TU)[u] += 1
            t0 += TU * WGS
            turn += 1
    assert sorted(seen) == list(range(tiles)), "the loop visits every tile exactly once"
    return tiles, len(per_turn), [tuple(per_turn[t]) for t in sorted(per_turn)]


def tile_regime(N, K):
    """Which edge of the tile loop a descriptor sits on."""
    tiles, turns, fill = tile_turns(N, K)
    if tiles == 1:
        return "1"
    if tiles < WGS:
        return "<64"
    if tiles == WGS:
        return "64"                   # every workgroup one tile, every second slot empty
    if tiles == WGS + 1:
        return "65"                   # ONE second slot in use
    if tiles < TU * WGS:
        return "65..127"
    if tiles == TU * WGS:
        return "128"                  # one full turn
    if tiles == TU * WGS + 1:
        return "129"                  # a second turn for one workgroup
    if tiles <= 2 * TU * WGS:
        return "129..256"
    return ">256"                     # a third turn


# ----------------------------------------------------------------------------------------------------- synthetic launches
def spec(N, K, **kw):
    """One synthetic Linear: N, K and the descriptor fields of rgbnm_linear_desc that are not offsets; zero_pad: the caller
    zeroes this descriptor's shadow segments before the launch (a `pair` descriptor's are always zeroed: its off-diagonal
    blocks are "left as the caller zeroed them"); block: the encoder block (chain_off / BLOCK_ELEMS) of a chain_kind."""
    s = dict(N=N, K=K, perm_heads=0, add_identity=0, ldn=0, pair=0, bias_mode=0, chain_kind=0, block=0, zero_pad=0)
    s.update(kw)
    return s


def chain_block(block):
    """The four Linears of one encoder block the chain images hold (E = 192, 3 heads): kinds 1 - 4."""
    return [spec(576, 192, perm_heads=3, chain_kind=1, block=block), spec(192, 192, bias_mode=1, chain_kind=2, block=block),
            spec(768, 192, chain_kind=3, block=block), spec(192, 768, bias_mode=1, chain_kind=4, block=block)]


# name -> the Linears of ONE launch.  Every launch mixes several descriptors whose segments lie next to each other.
SYNTH = {
    "small": [spec(1, 8), spec(8, 8, bias_mode=1), spec(31, 33), spec(32, 32, bias_mode=1), spec(33, 31), spec(40, 200),
              spec(64, 40)],
    "turns": [spec(256, 256), spec(264, 256, bias_mode=1), spec(512, 256), spec(520, 256), spec(160, 416), spec(96, 1376)],
    "ldn": [spec(1000, 192, bias_mode=1), spec(1000, 192, ldn=1000), spec(1000, 192, ldn=1008, bias_mode=1),
            spec(10, 192, ldn=16, zero_pad=1), spec(10, 33, ldn=16, zero_pad=1, bias_mode=1)],
    "pair": [spec(96, 96), spec(96, 96, pair=1), spec(288, 96, pair=1, bias_mode=1), spec(96, 384, pair=1, bias_mode=2),
             spec(288, 96, pair=1, bias_mode=2), spec(96, 96, pair=1, bias_mode=1)],
    "perm": [spec(576, 192, perm_heads=3), spec(1152, 384, perm_heads=6), spec(2304, 768, perm_heads=12), spec(40, 200)],
    "identity": [spec(192, 192, add_identity=1), spec(192, 384, add_identity=1, bias_mode=1), spec(384, 192, add_identity=1),
                 spec(192, 192), spec(576, 192, perm_heads=3, add_identity=1)],
    "bias": [spec(288, 96, bias_mode=0), spec(288, 96, bias_mode=1), spec(288, 96, bias_mode=2), spec(288, 96, pair=1),
             spec(288, 96, pair=1, bias_mode=1), spec(288, 96, pair=1, bias_mode=2), spec(33, 31, bias_mode=2),
             spec(1000, 192, bias_mode=2)],
}
CHAIN = {
    "depth1": chain_block(0) + [spec(40, 200, bias_mode=1)],
    "depth2": [spec(33, 31)] + chain_block(0) + [spec(264, 256, bias_mode=1)] + chain_block(1),
}


def _up(x, a):
    return -(-x // a) * a


class Launch:
    """Offsets, master and buffer sizes of one synthetic launch.
    master: fp32, NaN in every alignment gap, before the first and after the last segment; the weights are
    normal(0, 0.05)-like values from a seeded generator with put_specials on top, the biases plain values.
    Shadow / bias segments follow each other with at most the alignment gap (8 elements) between them."""

    def __init__(self, specs, seed, device="cpu", with_specials=True):
        self.specs = specs
        g = torch.Generator().manual_seed(seed)
        mo, so, bo = 8, 0, 0
        self.descs, self.segs, self.zero = [], [], []
        parts = []
        for i, s in enumerate(specs):
            N, K = s["N"], s["K"]
            W = torch.randn(N, K, generator=g) * 0.05
            if with_specials:
                put_specials(W, s["add_identity"], shift=7 * i + seed)
            w_off = mo
            parts.append((w_off, W.reshape(-1)))
            mo = _up(mo + N * K, 4) + 4 * (1 + i % 3)
            b_off = b2_off = 0
            if s["perm_heads"] or s["bias_mode"] == 1:
                b_off = mo
                parts.append((b_off, torch.randn(N, generator=g)))
                mo = _up(mo + N, 4) + 4
            elif s["bias_mode"] == 2:
                third = N // 3
                b_off = mo
                parts.append((b_off, torch.randn(third, generator=g)))
                mo = _up(mo + third, 4) + 4
                b2_off = mo
                parts.append((b2_off, torch.randn(N - 2 * third, generator=g)))
                mo = _up(mo + N - 2 * third, 4) + 4
            d = desc(N, K, w_off=w_off, b_off=b_off, b2_off=b2_off, perm_heads=s["perm_heads"], add_identity=s["add_identity"],
                     ldn=s["ldn"], pair=s["pair"], chain_kind=s["chain_kind"], chain_off=s["block"] * chain.BLOCK_ELEMS,
                     bias_mode=s["bias_mode"])
            e_ws, e_wst = shadow_extent(d)
            d.ws_off, d.wst_off = so, _up(so + e_ws, 8)
            so = _up(d.wst_off + e_wst, 8)
            self.segs += [("shadow", d.ws_off, e_ws, i), ("shadow", d.wst_off, e_wst, i)]
            if s["pair"] or s["zero_pad"]:
                self.zero += [(d.ws_off, e_ws), (d.wst_off, e_wst)]
            if s["perm_heads"] or s["bias_mode"]:
                nb = N * (2 if s["pair"] else 1)
                d.bperm_off = bo
                self.segs.append(("bias", bo, nb, i))
                bo = _up(bo + nb, 8)
            self.descs.append(d)
        self.master = torch.full((mo + 64,), float("nan"), dtype=F32)
        for off, v in parts:
            self.master[off:off + v.numel()] = v
            self.segs.append(("master", off, v.numel(), -1))
        self.master = self.master.to(device)
        self.shadow_elems, self.bias_elems = so, max(bo, 8)
        self.blocks = 1 + max(s["block"] for s in specs)

    def prefill(self, shadow):
        """Sentinel everywhere, zeros where a descriptor's segments are "left as the caller zeroed them"."""
        fill_sentinel(shadow)
        for off, n in self.zero:
            shadow[off:off + n] = 0
        return shadow


def disjoint(segs):
    """True if the (buffer, offset, elements, ...) segments of each buffer are pairwise disjoint."""
    by = {}
    for s in segs:
        by.setdefault(s[0], []).append((s[1], s[1] + s[2]))
    for v in by.values():
        v.sort()
        for (a0, a1), (b0, b1) in zip(v, v[1:]):
            if b0 < a1:
                return False
    return True


def desc_segments(descs, with_bias=True):
    """The segments a descriptor table reads and writes, for disjoint(): shadows (pads included), bias_perm, master."""
    segs = []
    for i, d in enumerate(descs):
        e_ws, e_wst = shadow_extent(d)
        segs += [("shadow", d.ws_off, e_ws, i), ("shadow", d.wst_off, e_wst, i), ("master", d.w_off, d.N * d.K, i)]
        if with_bias and (d.perm_heads > 0 or d.bias_mode):
            segs.append(("bias", d.bperm_off, d.N * (2 if d.pair and d.perm_heads <= 0 else 1), i))
        if d.perm_heads > 0 or d.bias_mode == 1:
            segs.append(("master", d.b_off, d.N, i))
        elif d.bias_mode == 2:
            segs += [("master", d.b_off, d.N // 3, i), ("master", d.b2_off, d.N - 2 * (d.N // 3), i)]
    return segs
