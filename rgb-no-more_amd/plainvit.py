"""Drop-in mirror of the reference `models/plainvit.py` ViT for `--domain DCT`, embed_type 1
(PatchEmbedding_DCT_Group, plainvit.py:157-218, :559-611), executing on hand-written HIP kernels.

* same constructor signature as `pvit.ViT(...)` (pipeline_utils.py:335-349) and the same 152 `state_dict()`
  keys / shapes / default init (parameter holders are ordinary nn.Linear / nn.LayerNorm modules, never called);
* `forward(y, cbcr) -> logits (B, n_classes) fp32`;
* compute dtype = the active autocast dtype (bf16 or fp16) or fp32 when autocast is off, so train.py's
  `--amp/--ampdtype` flags and its DDP loop work unchanged;
* one autograd node per stage (patch-embed, each encoder block, head) = one C-ABI call each; parameter
  gradients are ordinary leaf grads, so DDP's bucketed all-reduce (RCCL) overlaps with backward.

There is no fallback path: without librgbnm.so / a HIP device `forward` raises.
"""
import ctypes as C
import numpy as np
import math
import threading
import warnings
from collections import OrderedDict

import torch
from torch import nn

from . import dct_ops as dops
from . import lib as L
from .cls_transforms import LazyMixed
from .flatparams import FlatParamModule, align as _align


# ------------------------------------------------------------------ parameter-holder module tree
class ResidualAdd(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class MultiHeadAttention(nn.Module):
    def __init__(self, emb_size, num_heads, head_size, input_embed=-1, device="cpu", dtype=torch.float32):
        super().__init__()
        inner = num_heads * head_size
        self.qkv = nn.Linear(emb_size if input_embed < 0 else input_embed, inner * 3, device=device, dtype=dtype)
        self.projection = nn.Linear(inner, emb_size, device=device, dtype=dtype)


class PatchEmbedding_DCT_Group(nn.Module):
    """plainvit.py:157-218; only the parameters live here, compute is rgbnm_patch_embed_fwd."""

    def __init__(self, patch_size=16, emb_size=768, use_subblock=True, chroma_scale=2, device="cpu",
                 dtype=torch.float32):
        super().__init__()
        assert not (patch_size & (patch_size - 1)) and patch_size >= 2, \
            f"Patch size should be 2^n (n>0, n=int). Current value: {patch_size}"
        if patch_size != 16 or chroma_scale != 2 or not use_subblock:
            raise NotImplementedError("HIP path covers patch_size=16, 4:2:0, use_subblock=True (JPEG-Ti/S configs)")
        self.patch_size = patch_size
        fin = patch_size ** 2 + 2 * (patch_size // chroma_scale) ** 2
        self.projection = nn.Sequential(nn.Linear(fin, emb_size, device=device, dtype=dtype))
        # conv_Y is a plain attribute in the reference too (not a buffer, not in the state_dict)
        self.conv_Y = dops.generate_conversion_matrix(8, patch_size // 8, scale=True, dtype=torch.float32)


class PatchEmbedding_DCT_Separate_subblock(nn.Module):
    """plainvit.py:280-352 (ver=2 / embed_type 2 with use_subblock; train.py's default): Y tile -> Linear(256, E/6*4),
    Cb|Cr blocks -> Linear(128, E/6*2), GELU on the concatenation, residual Linear(E, E), sin-cos.  Parameter holder
    only; compute is _PatchEmbed2Fn (the same C-ABI GEMM / sub-block kernels as ver=1)."""

    def __init__(self, patch_size=16, emb_size=768, chroma_scale=2, device="cpu", dtype=torch.float32):
        super().__init__()
        assert not (patch_size & (patch_size - 1)) and patch_size >= 2, \
            f"Patch size should be 2^n (n>0, n=int). Current value: {patch_size}"
        if patch_size != 16 or chroma_scale != 2:
            raise NotImplementedError("HIP path covers patch_size=16, 4:2:0 (JPEG-Ti/S configs)")
        self.patch_size = patch_size
        kw = dict(device=device, dtype=dtype)
        # index 0 of each Sequential is the reference's parameter-free Rearrange
        self.projection_Y = nn.Sequential(nn.Identity(), nn.Linear(256, emb_size // 6 * 4, **kw))
        self.projection_C = nn.Sequential(nn.Identity(), nn.Linear(128, emb_size // 6 * 2, **kw))
        self.linearMix = nn.Linear(emb_size, emb_size, **kw)
        self.conv_Y = dops.generate_conversion_matrix(8, patch_size // 8, scale=True, dtype=torch.float32)


class PatchEmbedding_DCT_Separate(nn.Module):
    """plainvit.py:220-278 (ver=2 / embed_type 2 WITHOUT sub-block conversion): one Linear(64, E/6) per 8x8 block of the
    patch (Y_1..Y_4 in '(pdh pdw)' order, Cb, Cr), GELU on the concatenation, Linear(E, E), sin-cos.  Parameter holder; the
    reference registers LinearMix twice (as `LinearMix` and inside `projection`), so both state_dict keys exist here too.
    Compute is _PatchEmbedSepFn: the six small Linears run as ONE block-diagonal [E, 384] GEMM on the patch features."""

    def __init__(self, patch_size=16, emb_size=768, chroma_scale=2, device="cpu", dtype=torch.float32):
        super().__init__()
        assert not (patch_size & (patch_size - 1)) and patch_size >= 2, \
            f"Patch size should be 2^n (n>0, n=int). Current value: {patch_size}"
        assert patch_size // chroma_scale >= 8, \
            (f"Patch size for both Y and CbCr should be larger than 8 for this embedding method. Current patch size (Y): "
             f"{patch_size}, chroma scale: {chroma_scale}, patch_size (CbCr): {patch_size // chroma_scale}")
        if patch_size != 16 or chroma_scale != 2:
            raise NotImplementedError("HIP path covers patch_size=16, 4:2:0 (JPEG-Ti/S configs)")
        self.patch_size = patch_size
        kw = dict(device=device, dtype=dtype)
        nb = 6                                                # 4 luma + 2 chroma blocks per 16x16 patch
        self.LinearY = nn.ModuleList([nn.Linear(64, emb_size // nb, **kw) for _ in range(4)])
        self.LinearC = nn.ModuleList([nn.Linear(64, emb_size // nb, **kw) for _ in range(2)])
        self.PreMixActivation = nn.Identity()
        self.LinearMix = nn.Linear((emb_size // nb) * nb, emb_size, **kw)
        self.projection = nn.Sequential(self.PreMixActivation, self.LinearMix)


class PatchEmbedding_DCT_Concat(nn.Module):
    """plainvit.py:353-410 (ver=3 / embed_type 3): Y and CbCr are embedded SEPARATELY with the same 16x16 sub-block patches
    -- 14x14 luma tokens + 2 x 7x7 chroma tokens = 294 tokens, each with its own sin-cos table -- and concatenated along
    the token axis.  Parameter holder; compute is _PatchEmbedConcatFn."""

    def __init__(self, patch_size=16, emb_size=768, use_subblock=True, device="cpu", dtype=torch.float32):
        super().__init__()
        assert not (patch_size & (patch_size - 1)) and patch_size >= 2, \
            f"Patch size should be 2^n (n>0, n=int). Current value: {patch_size}"
        if patch_size != 16 or not use_subblock:
            raise NotImplementedError("HIP path covers patch_size=16 with sub-block conversion (JPEG-Ti/S configs)")
        self.patch_size = patch_size
        kw = dict(device=device, dtype=dtype)
        self.projectionY = nn.Sequential(nn.Identity(), nn.Linear(patch_size ** 2, emb_size, **kw))
        self.projectionC = nn.Sequential(nn.Identity(), nn.Linear(patch_size ** 2, emb_size, **kw))
        self.convMat = dops.generate_conversion_matrix(8, patch_size // 8, scale=True, dtype=torch.float32)
        self.conv_Y = self.convMat


def sincos_table(h, w, e, device="cpu"):
    """SinCosEmbedding (plainvit.py:90-121) as a constant (h*w, e) fp32 table."""
    hg, wg = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    fr = torch.log(torch.tensor(10000, dtype=torch.int32)) / (e // 4 - 1)
    fr = torch.exp(-torch.arange(e // 4, dtype=torch.float32) * fr)
    ph = torch.einsum("p,f->pf", hg.flatten().float(), fr)
    pw = torch.einsum("p,f->pf", wg.flatten().float(), fr)
    return torch.cat((pw.sin(), pw.cos(), ph.sin(), ph.cos()), dim=-1).contiguous().to(device)


# ------------------------------------------------------------------ per-forward state
CHAIN_MAX_DEPTH = 12        # blocks per launch of the one-launch encoder kernels (vit_chain.hip MAX_DEPTH: the argument segment)


class _Arena:
    """Activation / scratch buffers for one (B, dtype, grad) configuration with pre-built ctypes structs."""

    def __init__(self, model, B, cdtype, need_grad):
        dev = model._flat.device
        E, I, N, D = model.emb_size, model.inner, model.n_tokens, model.depth
        M = B * N
        T = cdtype
        self.B, self.cdtype, self.need_grad = B, cdtype, need_grad
        e = lambda *s, dt=T: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
        f32 = torch.float32
        self.cfg = L.VitCfg(L.dt_of(T), B, N, E, model.num_heads, 1e-5, 1.0 / math.sqrt(E))
        self.feat = e(M, 384)
        if model.embed_kind == "concat":
            self.featC = e(B * 98, 384)
            self.pe_ty, self.pe_tc = e(B * 196, E), e(B * 98, E)
        elif model.embed_kind != "group":
            self.pe_g, self.pe_gp = e(M, E), e(M, E)
            if need_grad:
                self.pe_dh = e(M, E)
        nx = D + 1 if need_grad else 2
        self.x = [e(M, E) for _ in range(nx)]
        nb = D if need_grad else 1
        self.blk = []
        for _ in range(nb):
            self.blk.append(dict(xn1=e(M, E), mean1=e(M, dt=f32), rstd1=e(M, dt=f32), qkv=e(M, 3 * I),
                                 lse=e(B * model.num_heads * N, dt=f32), attn=e(M, I), x_mid=e(M, E), xn2=e(M, E),
                                 mean2=e(M, dt=f32), rstd2=e(M, dt=f32), u=e(M, 4 * E), gl=e(M, 4 * E)))
        self.hmean, self.hrstd = e(M, dt=f32), e(M, dt=f32)
        self.pooled, self.h1 = e(B, E), e(B, E)
        ws_bytes = L.lib().rgbnm_vit_workspace_ex(C.byref(self.cfg), model._ncls_pad)      # the PADDED head width: its dW partials live here
        self.ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        if need_grad:
            self.du, self.dxn, self.dx_mid = e(M, 4 * E), e(M, E), e(M, E)
            self.dattn, self.dqkv = e(M, I), e(M, 3 * I)
            self.dx = [e(M, E), e(M, E)]
            self.da, self.dpooled = e(B, E), e(B, E)
            self.scratch = L.BlockScratch(self.du.data_ptr(), self.dxn.data_ptr(), self.dx_mid.data_ptr(),
                                          self.dattn.data_ptr(), self.dqkv.data_ptr(), self.ws.data_ptr(), ws_bytes)
        self.ws_bytes = ws_bytes
        # ---- built on first use, None until then: every lazily built member is named here and has ONE builder below
        self.chain_table = None      # host array of rgbnm_chain_block, built by the first one-launch forward (ViT._chain_forward)
        self.ws_blk = self.ws_head = self.hold_table = self.hold_table_host = self.scratch_blk = None      # build_hold
        self.du_blk = self.dxmid_blk = self.dqkv_blk = self.dx_blk = self.dattn_chain = self.lnpart = self.ws_chain = None     # build_chain_bwd
        self.chain_bwd_table = self.chain_bwd_dy = None     # build_chain_bwd: host array of rgbnm_chain_bwd_block and the dy it was built for
        self.drop_dy = self.drop_dxmid = None               # build_dropout
        self.acts = []
        for i in range(D):
            b = self.blk[i if need_grad else 0]
            xi, xo = (self.x[i], self.x[i + 1]) if need_grad else (self.x[i & 1], self.x[(i + 1) & 1])
            self.acts.append(L.BlockActs(xi.data_ptr(), b["xn1"].data_ptr(), b["mean1"].data_ptr(),
                                         b["rstd1"].data_ptr(), b["qkv"].data_ptr(), b["lse"].data_ptr(),
                                         b["attn"].data_ptr(), b["x_mid"].data_ptr(), b["xn2"].data_ptr(),
                                         b["mean2"].data_ptr(), b["rstd2"].data_ptr(), b["u"].data_ptr(),
                                         b["gl"].data_ptr(), xo.data_ptr()))

    def xbuf(self, i):
        return self.x[i] if self.need_grad else self.x[i & 1]

    def build_hold(self, m):
        """What the first held backward needs (_FwdState.begin_hold): the partial sums of every block now live until the end of the pass."""
        if self.ws_blk is not None:
            return
        dev = self.ws.device
        self.ws_blk = torch.empty(m.depth * self.ws_bytes, device=dev, dtype=torch.uint8)
        # ... and the head's three producers side by side (self.ws stays the patch embedding's)
        self.ws_head = torch.empty(L.lib().rgbnm_head_bwd_workspace(C.byref(self.cfg), m._ncls_pad), device=dev, dtype=torch.uint8)
        self.hold_table = torch.zeros(L.lib().rgbnm_reduce_hold_table_bytes(), device=dev, dtype=torch.uint8)
        # host record of what hold_table holds: allocated and freed WITH it (rgbnm.h), so a recycled device address
        # never inherits somebody else's "already uploaded"
        self.hold_table_host = torch.zeros(self.hold_table.numel(), dtype=torch.uint8)
        self.scratch_blk = [L.BlockScratch(self.du.data_ptr(), self.dxn.data_ptr(), self.dx_mid.data_ptr(), self.dattn.data_ptr(),
                                           self.dqkv.data_ptr(), self.ws_blk.data_ptr() + i * self.ws_bytes, self.ws_bytes)
                            for i in range(m.depth)]

    def build_chain_bwd(self, m, dy):
        """What the one-launch backward needs (ViT._chain_backward): per-block operand buffers, once, and the host array of
        rgbnm_chain_bwd_block, again whenever the last block's dy has moved."""
        if self.chain_bwd_table is not None and self.chain_bwd_dy == dy.data_ptr():
            return
        from . import chain as _chain
        D, dev = m.depth, self.ws.device
        if self.chain_bwd_table is None:
            M, E, I = self.B * m.n_tokens, m.emb_size, m.inner
            e = lambda *s, dt=self.cdtype: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
            self.du_blk = [e(M, 4 * E) for _ in range(D)]
            self.dxmid_blk = [e(M, E) for _ in range(D)]
            self.dqkv_blk = [e(M, 3 * I) for _ in range(D)]
            self.dx_blk = [e(M, E) for _ in range(D)]
            self.dattn_chain = e(M, I)
            self.lnpart = torch.empty(D, 2, self.B, 2, E, device=dev, dtype=torch.float32)
            # every block's split sums side by side (the weight-gradient GEMMs of several blocks run as one launch); the held
            # bracket's region serves when build_hold ran first
            self.ws_chain = self.ws_blk if self.ws_blk is not None else torch.empty(D * self.ws_bytes, device=dev, dtype=torch.uint8)
        blocks = (L.ChainBwdBlock * D)()
        for i in range(D):
            bp, ac = m._bparams[i], self.acts[i]
            blocks[i] = L.ChainBwdBlock(
                m._chain_img_bwd.data_ptr() + i * _chain.BLOCK_ELEMS * 2, bp.ln1_g, bp.ln2_g, ac.x_in, ac.mean1, ac.rstd1,
                ac.qkv, ac.lse, ac.attn, ac.x_mid, ac.mean2, ac.rstd2, ac.u,
                dy.data_ptr() if i == D - 1 else self.dx_blk[i + 1].data_ptr(),
                self.du_blk[i].data_ptr(), self.dxmid_blk[i].data_ptr(), self.dqkv_blk[i].data_ptr(), self.dx_blk[i].data_ptr(),
                self.lnpart[i, 0].data_ptr(), self.lnpart[i, 1].data_ptr())
        self.chain_bwd_table = blocks
        self.chain_bwd_dy = dy.data_ptr()

    def build_dropout(self, m):
        """Masked dy / d(x_mid) of one block's backward with dropout (ViT._begin_dropout)."""
        if self.need_grad and self.drop_dy is None:
            M, E = self.B * m.n_tokens, m.emb_size
            self.drop_dy = torch.empty(M, E, device=self.ws.device, dtype=self.cdtype)
            self.drop_dxmid = torch.empty(M, E, device=self.ws.device, dtype=self.cdtype)


class _Holder(threading.local):
    st = None                   # the _FwdState whose held-reduction bracket is open on this (autograd) thread


_HOLDER = _Holder()


class _FwdState:
    """Shared by the autograd nodes of one forward; hands the arena back to the pool when the graph dies."""

    def __init__(self, model, arena, gbuf):
        self.model, self.arena, self.gbuf = model, arena, gbuf
        self.prep_gen = model._prep_gen        # the prep this forward ran on (ViT._check_prep_gen, _ensure_block_shadows)
        self.ln_chain = False                  # per-operation forward: fc2 of block i also emits LN1 of block i+1 (ViT.forward sets it)
        self.holding = False                   # this state's held-reduction bracket is open (begin_hold .. end_hold / cancel_hold)
        self.drop = self.drop_seed = None      # dropout p > 0: per-block rgbnm_dropout structs and this forward's device seed
        self.chain_fwd = self.chain_bwd = False        # the one-launch kernel ran this pass's forward / backward data path
        self.dw_pending = []                   # chain backward: (block, BlockGrads, dy pointer) whose weight gradients are not launched yet
        self.pe_feat_ok = False                # arena.feat holds this forward's patch features (group embedding)
        self.pe_done = None                    # data_ptr of the dx0 whose patch-embedding gradients flush_dw has already computed

    # ---- held gradient reductions (rgbnm.h rgbnm_reduce_hold_*; ViT.defer_grad_reduction): opened after the head's backward,
    # closed in front of the patch embedding's, whose own reductions run at once (both nodes run on the same autograd thread:
    # the library's queues are thread-local)
    def begin_hold(self):
        m, a = self.model, self.arena
        gs = m._grad_sync
        if not m.defer_grad_reduction or (gs is not None and gs.bucket_elems < m._gflat.numel()):
            return                                     # somebody reads block gradients before the backward pass is over
        if self.grads_attached():
            return                                     # autograd adds each node's gradients to .grad as the node returns: reduce at once
        if not all(p.requires_grad for p in m._pe_params_list()):
            return                                     # a frozen patch embedding has no backward node to close the bracket
        a.build_hold(m)
        # one bracket per host thread (the library's queue is thread-local): a second forward state in the same backward pass
        # (two models, or one model applied twice) closes the bracket that is open -- its held reductions run now, its remaining
        # blocks reduce the ordinary way -- before it opens its own
        other = _HOLDER.st
        if other is not None and other is not self:
            other.end_hold()
        if L.lib().rgbnm_reduce_hold_begin() != 0:     # a bracket left open by a backward pass that died on this thread
            L.lib().rgbnm_reduce_hold_cancel()
            L.check(L.lib().rgbnm_reduce_hold_begin(), "reduce_hold_begin")
        self.holding = True
        _HOLDER.st = self

    def grads_attached(self):
        """True when autograd ADDS this backward's gradients to .grad tensors that already exist (gradient accumulation, or
        zero_grad(set_to_none=False)): the backward then writes a side buffer (FlatParamModule._grad_buffer), or .grad was attached
        by hand.  AccumulateGrad reads a node's gradients as soon as the node returns, so nothing of such a pass may be held."""
        m = self.model
        return self.gbuf.data_ptr() != m._gflat.data_ptr() or any(p.grad is not None for p in m._named.values())

    def end_hold(self):
        if self.holding:
            self.holding = False
            _HOLDER.st = None
            a = self.arena
            L.check(L.lib().rgbnm_reduce_hold_end(a.hold_table.data_ptr(), a.hold_table_host.data_ptr(), a.hold_table.numel(),
                                                  L.stream()), "reduce_hold_end")

    def cancel_hold(self):
        if self.holding:
            self.holding = False
            _HOLDER.st = None
            L.lib().rgbnm_reduce_hold_cancel()

    # ---- weight gradients behind the one-launch backward (_BlocksFn.backward): blocks wait in dw_pending until their group runs
    def dw_group(self):
        """(blocks per grouped weight-gradient launch, whether a LATER node may finish what this one leaves pending).
        AccumulateGrad, DDP's bucket hooks and any parameter hook read a node's gradients as soon as the node returns, so a node's
        weight-gradient GEMMs must have been launched by then (deferring them to block 0's node handed DDP stale
        buffers).  Only two readers wait: the held bracket, under which by contract nobody reads a block gradient before backward()
        returns, and the flat exchange, which owns the gradients and is told (`ready`) when a group has run -- both only while the
        backward writes the model's own flat buffer: a side buffer is ADDED to attached gradients by autograd, node by node.
        The more blocks share a launch the fewer token splits it has (rgbnm_vit_blocks_bwd_dw): everything a node may take at once
        it does, except under an exchange that is not held, whose transfers overlap the backward group by group."""
        m = self.model
        exchange = m._grad_sync is not None
        group = m.dw_group_overlapped if exchange and not self.holding else m.depth
        return min(group, CHAIN_MAX_DEPTH), self.gbuf.data_ptr() == m._gflat.data_ptr() and (self.holding or exchange)

    def flush_dw(self, whole_encoder):
        """ONE grouped launch for the blocks in dw_pending (descending), then their gradients are final: tell the exchange.
        whole_encoder: the caller is the node of all blocks, which returns a.dx_blk[0] -- the launch that holds every block may take
        the patch embedding's weight gradient along (same token axis: 252 + 4 = 256 tiles; its own launch and partial sums are gone)."""
        m, a = self.model, self.arena
        pend, self.dw_pending = self.dw_pending, []
        n = len(pend)
        scs = [L.BlockScratch(a.du_blk[i].data_ptr(), a.dxn.data_ptr(), a.dxmid_blk[i].data_ptr(), a.dattn_chain.data_ptr(),
                              a.dqkv_blk[i].data_ptr(), a.ws_chain.data_ptr() + i * a.ws_bytes, a.ws_bytes) for i, _, _ in pend]
        pa = (C.POINTER(L.BlockActs) * n)(*[C.pointer(a.acts[i]) for i, _, _ in pend])
        pg = (C.POINTER(L.BlockGrads) * n)(*[C.pointer(g) for _, g, _ in pend])
        ps = (C.POINTER(L.BlockScratch) * n)(*[C.pointer(x) for x in scs])
        pdy = (C.c_void_p * n)(*[d for _, _, d in pend])
        p2 = (C.c_void_p * n)(*[a.lnpart[i, 0].data_ptr() for i, _, _ in pend])
        p1 = (C.c_void_p * n)(*[a.lnpart[i, 1].data_ptr() for i, _, _ in pend])
        if (whole_encoder and n == m.depth and m.embed_kind == "group" and self.pe_feat_ok
                and all(p.requires_grad for p in m._pe_params_list())):
            gw, gb = self.pe_grads()
            L.check(L.lib().rgbnm_vit_blocks_bwd_dw_pe(C.byref(a.cfg), n, pa, pg, ps, pdy, p2, p1, a.dx_blk[0].data_ptr(),
                                                       a.feat.data_ptr(), gw.data_ptr(), gb.data_ptr(), a.ws.data_ptr(), a.ws_bytes,
                                                       L.stream()), "vit_blocks_bwd_dw_pe")
            self.pe_done = a.dx_blk[0].data_ptr()
        else:
            L.check(L.lib().rgbnm_vit_blocks_bwd_dw(C.byref(a.cfg), n, pa, pg, ps, pdy, p2, p1, L.stream()), "vit_blocks_bwd_dw")
        if m._grad_sync is not None:
            for i, _, _ in pend:
                m._grad_sync.ready(self.gbuf, m._block_names[i])

    # ---- what the four patch-embedding nodes' backwards share
    def pe_grads(self):
        return [self.model._gview(self.gbuf, n) for n in self.model._pe_names]

    def pe_return(self, grads, tail=()):
        """The last gradients of the step: flush the exchange (parallel.py); the node's return value (y, cbcr, st take none)."""
        m = self.model
        if m._grad_sync is not None:
            m._grad_sync.ready(self.gbuf, m._pe_names, last=True)
        return (None, None, None) + tuple(grads) + tail

    def __del__(self):
        try:
            self.model._release_arena(self.arena)
        except Exception:
            pass


# ------------------------------------------------------------------ autograd nodes
class _PatchEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, cbcr, st, w, b, lam=None):
        m, a = st.model, st.arena
        Hb, Wb = y.shape[2], y.shape[3]
        # lam: the device lambda of a cls_transforms.LazyMixed batch -- the mixup is applied while the sub-block kernel loads
        L.check(L.lib().rgbnm_patch_embed_fwd_mix(C.byref(a.cfg), L.dt_of(y.dtype), y.data_ptr(), cbcr.data_ptr(), L.ptr(lam),
                                                  m._conv16.data_ptr(), m._sh_ptr("pe", "ws"), b.data_ptr(),
                                                  m._pos.data_ptr(), a.feat.data_ptr(), a.xbuf(0).data_ptr(), Hb, Wb,
                                                  L.stream()), "patch_embed_fwd")
        ctx.st = st
        st.pe_feat_ok = True        # a.feat holds this forward's patch features (the encoder node may compute this node's dW from them)
        return a.xbuf(0).detach()   # fresh tensor object per call (arena buffers are reused across steps)

    @staticmethod
    def backward(ctx, dx0):
        st = ctx.st
        m, a = st.model, st.arena
        dx0 = dx0.contiguous()
        gw, gb = st.pe_grads()
        # held reductions (head, encoder blocks and this node's own: a.ws is no other node's region) run as ONE launch now, before
        # the exchange
        try:
            if st.pe_done != dx0.data_ptr():       # (else: computed by the encoder node's grouped launch)
                L.check(L.lib().rgbnm_patch_embed_bwd(C.byref(a.cfg), dx0.data_ptr(), a.feat.data_ptr(), gw.data_ptr(),
                                                      gb.data_ptr(), a.ws.data_ptr(), a.ws_bytes, L.stream()), "patch_embed_bwd")
        except BaseException:
            st.cancel_hold()
            raise
        st.end_hold()
        return st.pe_return((gw, gb), tail=(None,))


_PE2_NAMES = ["patchembed.projection_Y.1.weight", "patchembed.projection_Y.1.bias", "patchembed.projection_C.1.weight",
              "patchembed.projection_C.1.bias", "patchembed.linearMix.weight", "patchembed.linearMix.bias"]


class _PatchEmbed2Fn(torch.autograd.Function):
    """ver=2 patch embedding (reference: PatchEmbedding_DCT_Separate_subblock.forward, plainvit.py:326-352) on the
    C-ABI kernels:  feat = subblock(y, cbcr);  g = gelu([feat_Y Wy^T + by | feat_C Wc^T + bc])  (two GEMMs with the GELU
    epilogue writing column slices of g and gelu');  x0 = g (Wm + I)^T + bm + sincos  (one GEMM, sin-cos epilogue; the
    residual is folded into the operand shadow, rgbnm_linear_desc.add_identity)."""

    @staticmethod
    def forward(ctx, y, cbcr, st, wy, by, wc, bc, wm, bm):
        m, a = st.model, st.arena
        lib, dt, M, E = L.lib(), a.cfg.dtype, a.cfg.B * a.cfg.N, a.cfg.E
        Ey = E // 6 * 4
        Hb, Wb = y.shape[2], y.shape[3]
        if (Hb // 2) * (Wb // 2) != a.cfg.N:
            raise ValueError("expected a 28 x 28 block grid")
        es = a.feat.element_size()
        L.check(lib.rgbnm_subblock_embed(L.dt_of(y.dtype), dt, y.data_ptr(), cbcr.data_ptr(), m._conv16.data_ptr(),
                                         a.feat.data_ptr(), a.cfg.B, Hb, Wb, 0, L.stream()), "subblock_embed")
        g, gp = a.pe_g, a.pe_gp
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_GELU, a.feat.data_ptr(), 384, m._sh_ptr("peY", "ws"), 256, g.data_ptr(), E,
                                  by.data_ptr(), None, 0, gp.data_ptr(), E, None, 0, M, Ey, 256, 0, L.stream()), "pe2 Y")
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_GELU, a.feat.data_ptr() + 256 * es, 384, m._sh_ptr("peC", "ws"), 128,
                                  g.data_ptr() + Ey * es, E, bc.data_ptr(), None, 0, gp.data_ptr() + Ey * es, E, None,
                                  0, M, E - Ey, 128, 0, L.stream()), "pe2 C")
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_POS, g.data_ptr(), E, m._sh_ptr("peM", "ws"), E, a.xbuf(0).data_ptr(), E,
                                  bm.data_ptr(), None, 0, None, 0, m._pos.data_ptr(), a.cfg.N, M, E, E, 0, L.stream()),
                "pe2 mix")
        ctx.st = st
        return a.xbuf(0).detach()

    @staticmethod
    def backward(ctx, dx0):
        st = ctx.st
        st.end_hold()          # held reductions of the encoder blocks run now (before this node's own, and before the exchange)
        m, a = st.model, st.arena
        lib, dt, M, E = L.lib(), a.cfg.dtype, a.cfg.B * a.cfg.N, a.cfg.E
        Ey = E // 6 * 4
        dx0 = dx0.contiguous()
        es = a.feat.element_size()
        gr = st.pe_grads()
        ws, wsb = a.ws.data_ptr(), a.ws_bytes
        # d linearMix (the identity part of the shadow has no gradient)
        L.check(lib.rgbnm_gemm_tn(dt, dx0.data_ptr(), E, a.pe_g.data_ptr(), E, gr[4].data_ptr(), gr[5].data_ptr(), M, E,
                                  E, 0, 0, ws, wsb, L.stream()), "pe2 dWm")
        # dh = (dx0 (Wm + I)) * gelu'(h)
        dh = a.pe_dh
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_DGELU, dx0.data_ptr(), E, m._sh_ptr("peM", "wst"), E, dh.data_ptr(), E,
                                  None, a.pe_gp.data_ptr(), E, None, 0, None, 0, M, E, E, 0, L.stream()), "pe2 dh")
        L.check(lib.rgbnm_gemm_tn(dt, dh.data_ptr(), E, a.feat.data_ptr(), 384, gr[0].data_ptr(), gr[1].data_ptr(), M, Ey,
                                  256, 0, 0, ws, wsb, L.stream()), "pe2 dWy")
        L.check(lib.rgbnm_gemm_tn(dt, dh.data_ptr() + Ey * es, E, a.feat.data_ptr() + 256 * es, 384, gr[2].data_ptr(),
                                  gr[3].data_ptr(), M, E - Ey, 128, 0, 0, ws, wsb, L.stream()), "pe2 dWc")
        return st.pe_return(gr)


_PES_NAMES = ([f"patchembed.LinearY.{i}.{k}" for i in range(4) for k in ("weight", "bias")] +
              [f"patchembed.LinearC.{i}.{k}" for i in range(2) for k in ("weight", "bias")] +
              ["patchembed.LinearMix.weight", "patchembed.LinearMix.bias"])


class _PatchEmbedSepFn(torch.autograd.Function):
    """ver=2, use_subblock=False (reference: PatchEmbedding_DCT_Separate.forward, plainvit.py:257-278) on the C-ABI kernels:
    feat = the 2x2 luma blocks of a patch gathered as a 16x16 tile | Cb | Cr  (rgbnm_subblock_embed with the identity as
    conversion matrix: a pure index shuffle);  h = gelu(feat Wbd^T + b)  with Wbd the block-diagonal [E, 384] arrangement of
    the six Linear(64, E/6) (GELU epilogue);  x0 = h Wmix^T + bmix + sincos.  Backward: the dense [E, 384] weight gradient is
    computed by the dW GEMM and its six diagonal blocks are the parameter gradients."""

    @staticmethod
    def forward(ctx, y, cbcr, st, *params):
        m, a = st.model, st.arena
        lib, dt, M, E = L.lib(), a.cfg.dtype, a.cfg.B * a.cfg.N, a.cfg.E
        Hb, Wb = y.shape[2], y.shape[3]
        if (Hb // 2) * (Wb // 2) != a.cfg.N:
            raise ValueError("expected a 28 x 28 block grid")
        L.check(lib.rgbnm_subblock_embed(L.dt_of(y.dtype), dt, y.data_ptr(), cbcr.data_ptr(), m._eye16.data_ptr(),
                                         a.feat.data_ptr(), a.cfg.B, Hb, Wb, 0, L.stream()), "subblock_embed")
        wbd, bcat = m._sep_operands(a.cdtype)
        g, gp = a.pe_g, a.pe_gp
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_GELU, a.feat.data_ptr(), 384, wbd.data_ptr(), 384, g.data_ptr(), E,
                                  bcat.data_ptr(), None, 0, gp.data_ptr(), E, None, 0, M, E, 384, 0, L.stream()), "pe-sep blocks")
        bm = m._named["patchembed.LinearMix.bias"]
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_POS, g.data_ptr(), E, m._sh_ptr("peMix", "ws"), E, a.xbuf(0).data_ptr(), E,
                                  bm.data_ptr(), None, 0, None, 0, m._pos.data_ptr(), a.cfg.N, M, E, E, 0, L.stream()),
                "pe-sep mix")
        ctx.st = st
        return a.xbuf(0).detach()

    @staticmethod
    def backward(ctx, dx0):
        st = ctx.st
        st.end_hold()          # held reductions of the encoder blocks run now (before this node's own, and before the exchange)
        m, a = st.model, st.arena
        lib, dt, M, E = L.lib(), a.cfg.dtype, a.cfg.B * a.cfg.N, a.cfg.E
        dx0 = dx0.contiguous()
        gr = st.pe_grads()
        ws, wsb = a.ws.data_ptr(), a.ws_bytes
        L.check(lib.rgbnm_gemm_tn(dt, dx0.data_ptr(), E, a.pe_g.data_ptr(), E, gr[12].data_ptr(), gr[13].data_ptr(), M, E,
                                  E, 0, 0, ws, wsb, L.stream()), "pe-sep dWmix")
        dh = a.pe_dh
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_DGELU, dx0.data_ptr(), E, m._sh_ptr("peMix", "wst"), E, dh.data_ptr(), E,
                                  None, a.pe_gp.data_ptr(), E, None, 0, None, 0, M, E, E, 0, L.stream()), "pe-sep dh")
        dwbd = torch.empty(E, 384, device=dx0.device, dtype=torch.float32)
        dbcat = torch.empty(E, device=dx0.device, dtype=torch.float32)
        L.check(lib.rgbnm_gemm_tn(dt, dh.data_ptr(), E, a.feat.data_ptr(), 384, dwbd.data_ptr(), dbcat.data_ptr(), M, E,
                                  384, 0, 0, ws, wsb, L.stream()), "pe-sep dWbd")
        e6 = E // 6
        for i in range(6):                                   # diagonal blocks of the dense gradient = the six Linears
            gr[2 * i].copy_(dwbd[i * e6:(i + 1) * e6].index_select(1, m._sep_cols[i]))
            gr[2 * i + 1].copy_(dbcat[i * e6:(i + 1) * e6])
        return st.pe_return(gr)


_PE3_NAMES = ["patchembed.projectionY.1.weight", "patchembed.projectionY.1.bias", "patchembed.projectionC.1.weight",
              "patchembed.projectionC.1.bias"]


class _PatchEmbedConcatFn(torch.autograd.Function):
    """ver=3 (reference: PatchEmbedding_DCT_Concat.forward, plainvit.py:393-410).  The chroma tensor (B,2,14,14,8,8) is the
    luma layout of a batch of 2B single-plane images on a 14x14 block grid, so the same sub-block kernel combines its 2x2
    blocks into 16x16 tiles; token order 'b (c h w)' falls out of that view.  Two GEMMs with the sin-cos epilogue (periods
    196 and 49), then the two token groups are laid side by side per image."""

    @staticmethod
    def forward(ctx, y, cbcr, st, wy, by, wc, bc):
        m, a = st.model, st.arena
        lib, dt, E, B = L.lib(), a.cfg.dtype, a.cfg.E, a.cfg.B
        if y.shape[2:4] != (28, 28) or cbcr.shape[2:4] != (14, 14):
            raise ValueError("expected a 28 x 28 luma / 14 x 14 chroma block grid")
        idt = L.dt_of(y.dtype)
        zc = m._zero_chroma(2 * B, y.dtype)
        L.check(lib.rgbnm_subblock_embed(idt, dt, y.data_ptr(), cbcr.data_ptr(), m._conv16.data_ptr(), a.feat.data_ptr(),
                                         B, 28, 28, 0, L.stream()), "subblock_embed Y")
        L.check(lib.rgbnm_subblock_embed(idt, dt, cbcr.data_ptr(), zc.data_ptr(), m._conv16.data_ptr(), a.featC.data_ptr(),
                                         2 * B, 14, 14, 0, L.stream()), "subblock_embed C")
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_POS, a.feat.data_ptr(), 384, m._sh_ptr("peY3", "ws"), 256, a.pe_ty.data_ptr(), E,
                                  by.data_ptr(), None, 0, None, 0, m._pos.data_ptr(), 196, B * 196, E, 256, 0, L.stream()),
                "pe3 Y")
        L.check(lib.rgbnm_gemm_nt(dt, L.EPI_POS, a.featC.data_ptr(), 384, m._sh_ptr("peC3", "ws"), 256, a.pe_tc.data_ptr(), E,
                                  bc.data_ptr(), None, 0, None, 0, m._pos7.data_ptr(), 49, B * 98, E, 256, 0, L.stream()),
                "pe3 C")
        x0 = a.xbuf(0).view(B, 294, E)
        x0[:, :196].copy_(a.pe_ty.view(B, 196, E))
        x0[:, 196:].copy_(a.pe_tc.view(B, 98, E))
        ctx.st = st
        return a.xbuf(0).detach()

    @staticmethod
    def backward(ctx, dx0):
        st = ctx.st
        st.end_hold()          # held reductions of the encoder blocks run now (before this node's own, and before the exchange)
        m, a = st.model, st.arena
        lib, dt, E, B = L.lib(), a.cfg.dtype, a.cfg.E, a.cfg.B
        dxv = dx0.contiguous().view(B, 294, E)
        dty = dxv[:, :196].contiguous()
        dtc = dxv[:, 196:].contiguous()
        gr = st.pe_grads()
        ws, wsb = a.ws.data_ptr(), a.ws_bytes
        L.check(lib.rgbnm_gemm_tn(dt, dty.data_ptr(), E, a.feat.data_ptr(), 384, gr[0].data_ptr(), gr[1].data_ptr(),
                                  B * 196, E, 256, 0, 0, ws, wsb, L.stream()), "pe3 dWy")
        L.check(lib.rgbnm_gemm_tn(dt, dtc.data_ptr(), E, a.featC.data_ptr(), 384, gr[2].data_ptr(), gr[3].data_ptr(),
                                  B * 98, E, 256, 0, 0, ws, wsb, L.stream()), "pe3 dWc")
        return st.pe_return(gr)


class _BlocksFn(torch.autograd.Function):
    """Encoder blocks [lo, hi) as ONE autograd node.  ViT.forward applies it once as (0, depth) when the one-launch forward is
    switched on (single_encoder_node): the forward is then one C call (rgbnm_vit_chain_fwd), the backward one
    (rgbnm_vit_chain_bwd) plus the grouped weight-gradient launch(es) -- instead of twelve pass-through nodes whose Python /
    autograd bookkeeping was 1.3 ms of the 2.5 ms an eager step costs the host.  Otherwise (dropout, other dtypes and widths,
    single_encoder_node = False) it is applied once per block as (i, i + 1).  The one-launch kernels serve either layout: the node
    of block 0 runs the whole forward and the node of the last block the whole backward data path, the others hand buffers on;
    should a kernel not be eligible (an option switched off, no usable GELU table), every node runs the per-operation C entries
    for its own blocks."""

    @staticmethod
    def forward(ctx, x, st, lo, hi, *params):
        m, a = st.model, st.arena
        assert x.data_ptr() == a.xbuf(lo).data_ptr()
        ctx.st, ctx.lo, ctx.hi = st, lo, hi
        if st.drop is not None:
            # dropout p > 0 (ViT.train_dropout): the per-block entries with the masked epilogues (rgbnm.h rgbnm_vit_block_fwd_drop)
            for idx in range(lo, hi):
                L.check(L.lib().rgbnm_vit_block_fwd_drop(C.byref(a.cfg), C.byref(m._bparams[idx]), C.byref(a.acts[idx]),
                                                         C.byref(st.drop[idx]), L.stream()), "vit_block_fwd_drop")
            return a.xbuf(hi).detach()
        if lo == 0:
            st.chain_fwd = m._chain_forward(a)
        if not st.chain_fwd:
            # consecutive blocks are chained: fc2 of block i also emits LN1 of block i+1 (rgbnm.h, rgbnm_vit_block_fwd_chain)
            chain = st.ln_chain
            for idx in range(lo, hi):
                last = idx + 1 >= m.depth
                nxt_p = C.byref(m._bparams[idx + 1]) if chain and not last else None
                nxt_a = C.byref(a.acts[idx + 1]) if chain and not last else None
                L.check(L.lib().rgbnm_vit_block_fwd_chain(C.byref(a.cfg), C.byref(m._bparams[idx]), C.byref(a.acts[idx]),
                                                          1 if (chain and idx > 0) else 0, nxt_p, nxt_a, L.stream()), "vit_block_fwd")
        return a.xbuf(hi).detach()   # fresh tensor object per call (arena buffers are reused across steps)

    @staticmethod
    def backward(ctx, dy):
        st, lo, hi = ctx.st, ctx.lo, ctx.hi
        m, a = st.model, st.arena
        dy = dy.contiguous()
        grads = [[m._gview(st.gbuf, n) for n in m._block_names[i]] for i in range(lo, hi)]
        gs = [L.BlockGrads(*[t.data_ptr() for t in g]) for g in grads]
        try:
            if hi == m.depth:               # the first encoder node of the backward pass: the data path of EVERY block as one launch
                m._check_prep_gen(st)
                st.dw_pending = []
                st.chain_bwd = st.drop is None and m._chain_backward(a, dy)
                if not st.chain_bwd:
                    m._ensure_block_shadows(st)
            if st.chain_bwd:
                # only the weight-gradient GEMMs and their reductions are left: grouped launches (dw_group states the policy)
                group, later_node_may_finish = st.dw_group()
                for idx in range(hi - 1, lo - 1, -1):
                    # (no reference to the gradient views goes on st: autograd must be able to adopt them)
                    st.dw_pending.append((idx, gs[idx - lo], dy.data_ptr() if idx == hi - 1 else a.dx_blk[idx + 1].data_ptr()))
                    if len(st.dw_pending) >= group or idx == 0:
                        st.flush_dw(lo == 0 and hi == m.depth)
                if st.dw_pending and not later_node_may_finish:
                    st.flush_dw(False)
                dx = a.dx_blk[lo]
            else:
                cur = dy
                for idx in range(hi - 1, lo - 1, -1):
                    dx = a.dx[idx & 1]
                    if dx.data_ptr() == cur.data_ptr():
                        dx = a.dx[(idx + 1) & 1]
                    scratch = a.scratch_blk[idx] if st.holding else a.scratch
                    if st.drop is not None:
                        # the masks are regenerated from this forward's seed (st.drop_seed); dy_m / dxmid_m live in the arena
                        L.check(L.lib().rgbnm_vit_block_bwd_drop(C.byref(a.cfg), C.byref(m._bparams[idx]), C.byref(a.acts[idx]),
                                                                 C.byref(gs[idx - lo]), C.byref(scratch), C.byref(st.drop[idx]),
                                                                 cur.data_ptr(), dx.data_ptr(), L.stream()), "vit_block_bwd_drop")
                    else:
                        L.check(L.lib().rgbnm_vit_block_bwd(C.byref(a.cfg), C.byref(m._bparams[idx]), C.byref(a.acts[idx]),
                                                            C.byref(gs[idx - lo]), C.byref(scratch), cur.data_ptr(), dx.data_ptr(),
                                                            L.stream()), "vit_block_bwd")
                    if m._grad_sync is not None:        # this block's gradients are final: start their all-reduce now
                        m._grad_sync.ready(st.gbuf, m._block_names[idx])
                    cur = dx
        except BaseException:
            st.cancel_hold()                    # never leave the autograd thread's bracket open behind an exception
            raise
        # grads come back in BlockGrads field order; reorder to the order the params were passed in
        return (dx, None, None, None) + tuple(g[k] for i, g in zip(range(lo, hi), grads) for k in m._block_grad_perm[i])


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, st, *params):
        m, a = st.model, st.arena
        logits = torch.empty(a.B, m._ncls_pad, device=x.device, dtype=torch.float32)
        acts = L.HeadActs(x.data_ptr(), a.hmean.data_ptr(), a.hrstd.data_ptr(), a.pooled.data_ptr(),
                          a.h1.data_ptr(), logits.data_ptr())
        L.check(L.lib().rgbnm_head_fwd(C.byref(a.cfg), C.byref(m._hparams), C.byref(acts), L.stream()), "head_fwd")
        ctx.st, ctx.acts, ctx.x = st, acts, x
        ctx.set_materialize_grads(False)
        if m._ncls_pad != m.n_classes:
            return logits[:, :m.n_classes].contiguous()
        if a.cdtype == torch.float32:
            return logits
        # bf16 compute: a second, uninitialised [B, C] output in the compute dtype whose only purpose is to carry a gradient in
        # THAT dtype: cls_transforms.cross_entropy sends its dlogits back through it, so the bf16 head backward is not fed through
        # the fp32 round trip autograd's dtype check forces on a gradient of fp32 logits (two cast launches).  Any other loss uses
        # `logits` as always; gradients arriving on both edges are added.
        return logits, torch.empty(a.B, m._ncls_pad, device=x.device, dtype=a.cdtype)

    @staticmethod
    def backward(ctx, dlogits, dedge=None):
        st = ctx.st
        m, a = st.model, st.arena
        if dlogits is None and dedge is None:
            return (None,) * (2 + len(m._head_param_order))
        if dedge is not None:
            dlogits = dedge if dlogits is None else dedge + dlogits.to(dedge.dtype)
        names = m._head_names
        grads = [m._gview(st.gbuf, n) for n in names]
        padded = m._ncls_pad != m.n_classes
        if padded:                 # zero columns for the padded classes; dW2 / db2 land in padded buffers and are cut below
            dl = torch.zeros(a.B, m._ncls_pad, device=dlogits.device, dtype=a.cdtype)
            dl[:, :m.n_classes].copy_(dlogits)
            dw2p = torch.empty(m._ncls_pad, m.emb_size, device=dlogits.device, dtype=torch.float32)
            db2p = torch.empty(m._ncls_pad, device=dlogits.device, dtype=torch.float32)
            ptrs = [t.data_ptr() for t in grads]
            ptrs[names.index("classhead.ch_linear2.weight")] = dw2p.data_ptr()
            ptrs[names.index("classhead.ch_linear2.bias")] = db2p.data_ptr()
            g = L.HeadGrads(*ptrs)
        else:
            dl = dlogits.to(a.cdtype).contiguous()
            g = L.HeadGrads(*[t.data_ptr() for t in grads])
        dx = a.dx[0]
        if not padded:
            st.begin_hold()        # the bracket opens in front of the head: its own split sums join the one launch at the end
        ws = a.ws_head if st.holding else a.ws
        try:
            L.check(L.lib().rgbnm_head_bwd(C.byref(a.cfg), C.byref(m._hparams), C.byref(ctx.acts), C.byref(g),
                                           dl.data_ptr(), a.da.data_ptr(), a.dpooled.data_ptr(), dx.data_ptr(),
                                           ws.data_ptr(), ws.numel(), L.stream()), "head_bwd")
            if padded:             # (the padded head reduces at once: its gradients are cut out of the padded buffers here)
                grads[names.index("classhead.ch_linear2.weight")].copy_(dw2p[:m.n_classes])
                grads[names.index("classhead.ch_linear2.bias")].copy_(db2p[:m.n_classes])
            if m._grad_sync is not None:
                m._grad_sync.ready(st.gbuf, names)
        except BaseException:
            st.cancel_hold()
            raise
        if padded:
            st.begin_hold()
        return (dx, None) + tuple(grads[k] for k in m._head_grad_perm)      # HeadGrads field order -> the order the params were passed in


# ------------------------------------------------------------------ the model
class ViT(FlatParamModule):
    """Vision Transformer on DCT coefficients -- same ctor as the reference `ViT` (plainvit.py:559-599).

    defer_grad_reduction (default False): when True the split-sum reductions of the encoder blocks' weight / LayerNorm
    gradients are held during the backward pass and run as one launch in front of the patch embedding's backward (rgbnm.h,
    rgbnm_reduce_hold_*): parameter gradients of the blocks are then final only when `backward()` returns.  Safe with no
    gradient exchange or with FlatGradSync's single all-reduce after the backward; NOT with torch DDP or any hook that reads
    `.grad` during the backward (leave it False there).  A backward whose gradients autograd adds to `.grad` tensors that are still
    attached (gradient accumulation, `zero_grad(set_to_none=False)`) reads them node by node: the hold is off for that pass
    (_FwdState.grads_attached) and every node reduces at once -- the same bits, a few more launches."""
    defer_grad_reduction = False
    dw_group_overlapped = 4        # blocks per grouped weight-gradient launch while gradient slices are exchanged during the backward
    single_encoder_node = True     # all blocks as one autograd node when the one-launch forward is on (_BlocksFn); False: one node per block
    # training with drop_p > 0: False refuses (NotImplementedError); True runs the reference's three dropout sites per block on the device
    # (rgbnm.h, dropout mask contract): masks from this library's Philox stream, not torch's, and the per-block kernels instead of
    # the one-launch encoder
    train_dropout = False
    last_dropout_seed = None       # device int64 tensor: the seed of the latest training forward with dropout (the masks: rgbnm.h)

    def __init__(self, in_channels: int = 3, patch_size: int = 16, emb_size: int = 768, input_embed: int = -1,
                 depth: int = 12, n_classes: int = 1000, drop_p=0.1, pixel_space="RGB", ver=1, use_subblock=True,
                 device="cpu", dtype=torch.float32, num_heads: int = 8, head_size: int = 64, **kwargs):
        super().__init__()
        if pixel_space.lower() not in ("dct", "rgb2dct"):
            raise NotImplementedError("rgb-no-more_amd implements the --domain DCT path only")
        if ver not in (1, 2, 3):
            raise NotImplementedError("ver must be 1 (PatchEmbedding_DCT_Group), 2 (PatchEmbedding_DCT_Separate / "
                                      "_Separate_subblock) or 3 (PatchEmbedding_DCT_Concat)")
        if ver in (1, 3) and not use_subblock:
            raise NotImplementedError("embed_type 1 / 3 without sub-block conversion are not in any reference config")
        # nn.Dropout(drop_p) of plainvit.py:489, 515, 525 is the identity in eval mode: a model built with the constructor's default
        # (0.1) evaluates fine; TRAINING with p > 0 (train.py --drop) needs train_dropout = True, else forward() refuses
        if not 0.0 <= float(drop_p) < 1.0:
            raise ValueError("dropout probability has to be in [0, 1)")
        self.drop_p = float(drop_p)
        if head_size != 64 or emb_size not in (192, 384, 512, 768, 1024) or input_embed >= 0:
            raise NotImplementedError("HIP kernels cover head_size 64 and emb_size 192 / 384 (JPEG-Ti / JPEG-S; tuned) and "
                                      "512 / 768 / 1024 (vitb / vitl of utils/configs.py:104-122; generic kernels)")
        if dtype != torch.float32:
            raise NotImplementedError("parameters are fp32 masters; choose bf16 compute with autocast")
        if n_classes < 1:
            raise ValueError("n_classes must be positive")
        self.pixel_space = pixel_space
        self.emb_size, self.depth, self.n_classes = emb_size, depth, n_classes
        # the head GEMMs move 16-byte rows: a class count that is not a multiple of 8 is padded INSIDE (operand shadows, bias,
        # logits and their gradient carry zero columns; parameters, state_dict and the returned logits keep the real count)
        self._ncls_pad = (n_classes + 7) // 8 * 8
        self.num_heads, self.inner = num_heads, num_heads * head_size
        self.n_tokens = 294 if ver == 3 else 196          # ver 3: 14x14 luma + 2 x 7x7 chroma tokens
        E = emb_size
        kw = dict(device=device, dtype=dtype)
        self.ver = ver
        self.embed_kind = {1: "group", 3: "concat"}.get(ver, "sep_sub" if use_subblock else "sep")
        self.patchembed = {"group": lambda: PatchEmbedding_DCT_Group(patch_size, E, use_subblock, **kw),
                           "sep_sub": lambda: PatchEmbedding_DCT_Separate_subblock(patch_size, E, **kw),
                           "sep": lambda: PatchEmbedding_DCT_Separate(patch_size, E, **kw),
                           "concat": lambda: PatchEmbedding_DCT_Concat(patch_size, E, use_subblock, **kw)}[self.embed_kind]()
        blocks = []
        for _ in range(depth):
            att = ResidualAdd(nn.Sequential(OrderedDict([
                ("eb_lrnorm1", nn.LayerNorm(E, **kw)),
                ("eb_mha", MultiHeadAttention(E, num_heads, head_size, **kw)),
                ("eb_drop1", nn.Identity())])))
            ffn = ResidualAdd(nn.Sequential(OrderedDict([
                ("eb_lrnorm2", nn.LayerNorm(E, **kw)),
                ("eb_ffb", nn.Sequential(nn.Linear(E, 4 * E, **kw), nn.Identity(), nn.Identity(),
                                         nn.Linear(4 * E, E, **kw))),
                ("eb_drop2", nn.Identity())])))
            blocks.append(nn.Sequential(att, ffn))
        self.encoder = nn.Sequential(*blocks)
        self.classhead = nn.Sequential(OrderedDict([
            ("ch_lrnorm", nn.LayerNorm(E, **kw)), ("ch_gap", nn.Identity()),
            ("ch_linear1", nn.Linear(E, E, **kw)), ("ch_tanh", nn.Identity()),
            ("ch_linear2", nn.Linear(E, n_classes, **kw))]))
        self._flat = None
        self._arenas = {}
        self.compute_dtype = None      # None: follow autocast; or force torch.float32 / torch.bfloat16 / torch.float16
        # host state that lives as long as the model; what is tied to the device or to the Parameter objects is _flatten's
        self._prep_gen = 0             # counts _prep calls: the shadows and the chain images are model-global (_check_prep_gen)
        self._warned_prep_gen = self._warned_chain_forward = self._warned_chain_backward = False      # each warning is given once
        self._b2pad = self._abp = self._pe_params = None      # reset by every _flatten, which see

    # ---------------------------------------------------------------- flat buffers / shadows
    def _names(self):
        return [n for n, _ in self.named_parameters()]

    def _flatten(self):
        """(Re)pack every parameter into one fp32 buffer (256-element aligned segments) and describe the
        Linear layers for rgbnm_prep_weights.  Called lazily; survives .to(), load_state_dict (in-place copy)."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.RgbnmError("model parameters must live on a HIP device (no CPU fallback)")
        params = self._pack_parameters()
        offs = self._offs
        # what was built for the old device or from the old name -> Parameter map (`_named`) goes with them, as _arenas does below:
        # the padded head's bias buffer, the block parameters in _BlocksFn's argument order, the patch embedding's parameters
        self._b2pad = self._abp = self._pe_params = None
        # ---- Linear descriptors + shadow layout
        if self.embed_kind == "group":
            lin = [("pe", "patchembed.projection.0", 0)]
        elif self.embed_kind == "sep_sub":
            lin = [("peY", "patchembed.projection_Y.1", 0), ("peC", "patchembed.projection_C.1", 0),
                   ("peM", "patchembed.linearMix", 0)]
        elif self.embed_kind == "sep":
            lin = [("peMix", "patchembed.LinearMix", 0)]
        else:
            lin = [("peY3", "patchembed.projectionY.1", 0), ("peC3", "patchembed.projectionC.1", 0)]
        for i in range(self.depth):
            lin += [(f"qkv{i}", f"encoder.{i}.0.fn.eb_mha.qkv", self.num_heads),
                    (f"proj{i}", f"encoder.{i}.0.fn.eb_mha.projection", 0),
                    (f"fc1{i}", f"encoder.{i}.1.fn.eb_ffb.0", 0), (f"fc2{i}", f"encoder.{i}.1.fn.eb_ffb.3", 0)]
        lin += [("h1", "classhead.ch_linear1", 0), ("h2", "classhead.ch_linear2", 0)]
        descs = (L.LinearDesc * len(lin))()
        self._sh_off, so, bo = {}, 0, 0
        # one-launch encoder kernels (chain.py): rgbnm_prep_weights_chain writes a block Linear straight into the chain images
        chain_ok = self.emb_size == 192 and self.num_heads == 3 and self.n_tokens == 196
        from . import chain as _chain
        kinds = {"eb_mha.qkv": 1, "eb_mha.projection": 2, "eb_ffb.0": 3, "eb_ffb.3": 4}
        for k, (key, name, ph) in enumerate(lin):
            ck = kinds[name.split(".fn.")[1]] if chain_ok and name.startswith("encoder.") else 0
            coff = int(name.split(".")[1]) * _chain.BLOCK_ELEMS if ck else 0
            Nn, Kk = self._shapes[name + ".weight"]
            Np = self._ncls_pad if key == "h2" else Nn          # shadow rows / transposed-shadow stride (padded class count)
            ws, wst = so, so + _align(Np * Kk)
            so = wst + _align(Np * Kk)
            bp = bo
            if ph:
                bo += _align(Nn)
            descs[k] = L.LinearDesc(offs[name + ".weight"], offs[name + ".bias"], ws, wst, bp, Nn, Kk, ph,
                                    1 if key == "peM" else 0, Np if Np != Nn else 0, 0, ck, coff)
            self._sh_off[key] = (ws, wst, bp)
        self._ndesc, self._sh_total = len(lin), so
        self._descs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        self._bias_perm = torch.zeros(max(bo, 1), device=dev, dtype=torch.float32)
        self._shadow = {}
        self._shadow_gen = {}          # per dtype: the _prep_gen of the latest prep that wrote the block Linears' shadows (not skipped)
        if self.embed_kind == "sep":
            # feature column of coefficient (p1, p2) of luma block (pdh, pdw) in the 16x16 tile that the sub-block kernel emits
            self._eye16 = torch.eye(16, device=dev, dtype=torch.float32)
            p1, p2 = torch.meshgrid(torch.arange(8), torch.arange(8), indexing="ij")
            cols = [((pdh * 8 + p1) * 16 + pdw * 8 + p2).reshape(-1) for pdh in range(2) for pdw in range(2)]
            cols += [256 + torch.arange(64), 320 + torch.arange(64)]
            self._sep_cols = [c.to(dev) for c in cols]
            self._sep_cache = {}
        else:
            self._conv16 = self.patchembed.conv_Y.to(dev).contiguous()
        # one-launch encoder kernels: the two chain images (forward: [N, K] orientation, backward: transposed), rewritten every step
        # by rgbnm_prep_weights_chain.  _chain_idx stays the eligibility flag older code tests; the index TABLES that document the
        # layout (chain.py) are only built on demand (_chain_index_tables: tests compare the kernel's arithmetic with them)
        self._chain_idx = None
        self._chain_refused = False
        if chain_ok:
            assert _chain.BLOCK_ELEMS == L.lib().rgbnm_chain_image_elems()
            self._chain_idx = True
            self._chain_img = torch.zeros(self.depth * _chain.BLOCK_ELEMS, device=dev, dtype=torch.bfloat16)
            self._chain_img_bwd = torch.zeros(self.depth * _chain.BLOCK_ELEMS, device=dev, dtype=torch.bfloat16)
        self._pos = sincos_table(14, 14, self.emb_size, dev)
        self._pos7 = sincos_table(7, 7, self.emb_size, dev) if self.embed_kind == "concat" else None
        self._zc = {}
        self._build_names()
        self._arenas = {}
        # set-up call (synchronises once per device): GELU table of the fused FeedForwardBlock forward (rgbnm.h)
        L.check(L.lib().rgbnm_gelu_table_init(L.stream()), "gelu_table_init")

    def _zero_chroma(self, n, dtype):
        """(n, 2, 7, 7, 8, 8) zeros: the chroma argument of the sub-block kernel when the chroma planes themselves are
        embedded as luma (ver=3); its 128 output features are not used."""
        k = (n, dtype)
        if k not in self._zc:
            self._zc[k] = torch.zeros(n, 2, 7, 7, 8, 8, device=self._flat.device, dtype=dtype)
        return self._zc[k]

    def _sep_operands(self, cdtype):
        """Block-diagonal [E, 384] operand of the six per-block Linears (+ concatenated bias) for this step."""
        E, e6 = self.emb_size, self.emb_size // 6
        key = cdtype
        if key not in self._sep_cache:
            self._sep_cache[key] = (torch.zeros(E, 384, device=self._flat.device, dtype=cdtype),
                                    torch.zeros(E, device=self._flat.device, dtype=torch.float32))
        wbd, bcat = self._sep_cache[key]
        named = self._named
        for i in range(6):
            mod = f"patchembed.LinearY.{i}" if i < 4 else f"patchembed.LinearC.{i - 4}"
            wbd[i * e6:(i + 1) * e6].index_copy_(1, self._sep_cols[i], named[mod + ".weight"].detach().to(cdtype))
            bcat[i * e6:(i + 1) * e6].copy_(named[mod + ".bias"].detach())
        return wbd, bcat

    def _build_names(self):
        """Parameter names in the field order of BlockGrads / HeadGrads, and the groups the backward finishes in order (head,
        blocks depth-1 .. 0, patch embedding) -- the order parallel.FlatGradSync sees them.  Pure naming: works on CPU."""
        self._block_names, self._block_param_order, self._bparams_by_dtype = [], [], {}
        for i in range(self.depth):
            a, b = f"encoder.{i}.0.fn.", f"encoder.{i}.1.fn."
            self._block_names.append([a + "eb_lrnorm1.weight", a + "eb_lrnorm1.bias", b + "eb_lrnorm2.weight",
                                      b + "eb_lrnorm2.bias", a + "eb_mha.qkv.weight", a + "eb_mha.qkv.bias",
                                      a + "eb_mha.projection.weight", a + "eb_mha.projection.bias",
                                      b + "eb_ffb.0.weight", b + "eb_ffb.0.bias", b + "eb_ffb.3.weight",
                                      b + "eb_ffb.3.bias"])
            self._block_param_order.append([n for n in self._names() if n.startswith(f"encoder.{i}.")])
        self._head_names = ["classhead.ch_lrnorm.weight", "classhead.ch_lrnorm.bias", "classhead.ch_linear1.weight",
                            "classhead.ch_linear1.bias", "classhead.ch_linear2.weight", "classhead.ch_linear2.bias"]
        self._head_param_order = [n for n in self._names() if n.startswith("classhead.")]
        self._pe_names = {"group": ["patchembed.projection.0.weight", "patchembed.projection.0.bias"], "sep_sub": _PE2_NAMES,
                          "sep": _PES_NAMES, "concat": _PE3_NAMES}[self.embed_kind]
        # the kernels hand gradients back in field order, autograd wants them in the order the parameters were passed in
        # (_block_param_order / _head_param_order): out[j] = grads[perm[j]]
        self._block_grad_perm = [[names.index(n) for n in order] for names, order in zip(self._block_names, self._block_param_order)]
        self._head_grad_perm = [self._head_names.index(n) for n in self._head_param_order]

    def grad_ready_order(self):
        """[(names, last)] in the order the autograd nodes report finished gradients to the gradient exchange."""
        if not hasattr(self, "_head_names"):
            self._build_names()
        return ([(self._head_names, False)] + [(self._block_names[i], False) for i in reversed(range(self.depth))] +
                [(self._pe_names, True)])

    def _pe_params_list(self):
        if self._pe_params is None:
            self._pe_params = [p for n, p in self._named.items() if n.startswith("patchembed.")]
        return self._pe_params

    def _all_block_params(self):
        """The block parameters in the order the node of all blocks takes them (_BlocksFn as (0, depth))."""
        if self._abp is None:
            self._abp = [self._named[n] for order in self._block_param_order for n in order]
        return self._abp

    def _pptr(self, name):
        return self._flat.data_ptr() + self._offs[name] * 4

    def _sh_ptr(self, key, which):
        sh = self._shadow[self._cur_dtype]
        ws, wst, _ = self._sh_off[key]
        return sh.data_ptr() + (ws if which == "ws" else wst) * sh.element_size()

    def _chain_index_tables(self):
        """(forward, backward) int32 gather tables over the operand shadows (chain.py): dst[i] = shadow[idx[i]] -- the definition of
        the chain images that rgbnm_prep_weights_chain's address arithmetic is tested against."""
        from . import chain as _chain
        dev = self._flat.device
        idx = np.concatenate([_chain.block_index(self._sh_off[f"qkv{i}"][0], self._sh_off[f"proj{i}"][0],
                                                 self._sh_off[f"fc1{i}"][0], self._sh_off[f"fc2{i}"][0]) for i in range(self.depth)])
        idb = np.concatenate([_chain.block_index_bwd(self._sh_off[f"qkv{i}"][1], self._sh_off[f"proj{i}"][1],
                                                     self._sh_off[f"fc1{i}"][1], self._sh_off[f"fc2{i}"][1])
                              for i in range(self.depth)])
        assert max(idx.max(), idb.max()) < 2 ** 31
        return torch.from_numpy(idx.astype(np.int32)).to(dev), torch.from_numpy(idb.astype(np.int32)).to(dev)

    def _prep(self, cdtype, chains=True, shadows=False):
        """fp32 masters -> operand shadows (cast, qkv de-interleave, transposes) and, for the one-launch encoder kernels, their
        chain images -- ONE launch per step.  chains=False: a step on the per-block kernels (dropout): shadows only.
        shadows=True: never skip the block Linears' shadows (_ensure_block_shadows)."""
        if cdtype not in self._shadow:
            self._shadow[cdtype] = torch.zeros(self._sh_total, device=self._flat.device, dtype=cdtype)
        self._cur_dtype = cdtype
        self._prep_gen += 1        # (the shadows and the chain images are model-global: see _check_prep_gen)
        chain = chains and cdtype == torch.bfloat16 and self._chain_idx is not None
        img_f = self._chain_img.data_ptr() if chain and L.lib().rgbnm_get_option(b"fwd_chain") else None
        img_b = (self._chain_img_bwd.data_ptr() if chain and L.lib().rgbnm_get_option(b"bwd_chain") and torch.is_grad_enabled()
                 else None)
        # the block Linears' own shadows are only read by the per-operation kernels: skipped while both directions run as chains
        skip = bool(img_f and (img_b or not torch.is_grad_enabled()) and not self._chain_refused and not shadows)
        if not skip:
            self._shadow_gen[cdtype] = self._prep_gen
        L.check(L.lib().rgbnm_prep_weights_chain(L.dt_of(cdtype), self._descs_dev.data_ptr(), self._ndesc, self._flat.data_ptr(),
                                                 self._shadow[cdtype].data_ptr(), self._bias_perm.data_ptr(), img_f, img_b,
                                                 1 if skip else 0, L.stream()), "prep_weights")
        if cdtype not in self._bparams_by_dtype:
            bps = []
            for i in range(self.depth):
                a, b = f"encoder.{i}.0.fn.", f"encoder.{i}.1.fn."
                bps.append(L.BlockParams(
                    self._pptr(a + "eb_lrnorm1.weight"), self._pptr(a + "eb_lrnorm1.bias"),
                    self._pptr(b + "eb_lrnorm2.weight"), self._pptr(b + "eb_lrnorm2.bias"),
                    self._bias_perm.data_ptr() + self._sh_off[f"qkv{i}"][2] * 4,
                    self._pptr(a + "eb_mha.projection.bias"), self._pptr(b + "eb_ffb.0.bias"),
                    self._pptr(b + "eb_ffb.3.bias"),
                    self._sh_ptr(f"qkv{i}", "ws"), self._sh_ptr(f"qkv{i}", "wst"),
                    self._sh_ptr(f"proj{i}", "ws"), self._sh_ptr(f"proj{i}", "wst"),
                    self._sh_ptr(f"fc1{i}", "ws"), self._sh_ptr(f"fc1{i}", "wst"),
                    self._sh_ptr(f"fc2{i}", "ws"), self._sh_ptr(f"fc2{i}", "wst")))
            if self._ncls_pad != self.n_classes and self._b2pad is None:
                self._b2pad = torch.zeros(self._ncls_pad, device=self._flat.device, dtype=torch.float32)
            b2 = self._b2pad.data_ptr() if self._ncls_pad != self.n_classes else self._pptr("classhead.ch_linear2.bias")
            hp = L.HeadParams(self._pptr("classhead.ch_lrnorm.weight"), self._pptr("classhead.ch_lrnorm.bias"),
                              self._pptr("classhead.ch_linear1.bias"), b2,
                              self._sh_ptr("h1", "ws"), self._sh_ptr("h1", "wst"), self._sh_ptr("h2", "ws"),
                              self._sh_ptr("h2", "wst"), self._ncls_pad, 0)
            self._bparams_by_dtype[cdtype] = (bps, hp)
        self._bparams, self._hparams = self._bparams_by_dtype[cdtype]
        if self._ncls_pad != self.n_classes:
            self._b2pad[:self.n_classes].copy_(self._named["classhead.ch_linear2.bias"].detach())

    def _check_prep_gen(self, st):
        """The operand shadows / chain images a backward reads are the ones of the LATEST forward (one set per model, rewritten by
        every forward).  A forward between a training forward and its backward is harmless while the weights are the same, but
        after an optimizer step (or swapped-in weights) that backward would run against the newer weights: say so."""
        if st.prep_gen != self._prep_gen and not self._warned_prep_gen:
            self._warned_prep_gen = True
            warnings.warn("rgb-no-more_amd: another forward of this model ran between a forward and its backward; the backward uses the "
                          "weight operands of the LATEST forward (identical unless the parameters changed in between)", RuntimeWarning,
                          stacklevel=3)

    def _ensure_block_shadows(self, st):
        """A backward on the per-operation kernels reads the block Linears' shadows.  The prep of its forward skipped them if both
        chain kernels were switched on then; with bwd_chain switched off since, they hold the weights of some earlier step (or
        nothing): write them now, from the same masters, as the refusal path of _chain_backward does."""
        if self._shadow_gen.get(st.arena.cdtype, 0) < st.prep_gen:
            self._prep(st.arena.cdtype, shadows=True)

    def _warn_chain_refused(self, which):
        """The library refused the one-launch encoder kernel for a model that looks eligible from here (E = 192, 3 heads, bf16,
        option on): no usable GELU table.  The per-operation kernels run instead -- same results, about half the
        speed -- so say it once instead of silently."""
        key = "_warned_chain_" + which          # _warned_chain_forward / _warned_chain_backward (__init__)
        if not self.__dict__[key]:
            self.__dict__[key] = True
            warnings.warn(f"rgb-no-more_amd: the one-launch encoder {which} kernel refused this model (no GELU "
                          f"table); running the per-operation kernels (about 2x slower)", RuntimeWarning, stacklevel=3)

    def _chain_forward(self, a):
        """Run all encoder blocks as one launch into arena `a` (rgbnm_vit_chain_fwd); False = not eligible (per-block path)."""
        if a.cdtype != torch.bfloat16 or self._chain_idx is None or not L.lib().rgbnm_get_option(b"fwd_chain"):
            return False
        if a.chain_table is None:
            from . import chain as _chain
            blocks = (L.ChainBlock * self.depth)()
            for i in range(self.depth):
                bp, ac = self._bparams[i], a.acts[i]
                blocks[i] = L.ChainBlock(self._chain_img.data_ptr() + i * _chain.BLOCK_ELEMS * 2,
                                         bp.ln1_g, bp.ln1_b, bp.ln2_g, bp.ln2_b, bp.bqkv_perm, bp.bproj, bp.b1, bp.b2,
                                         ac.xn1, ac.mean1, ac.rstd1, ac.qkv, ac.lse, ac.attn, ac.x_mid, ac.xn2, ac.mean2, ac.rstd2,
                                         ac.u, ac.gl, ac.x_out)
            a.chain_table = blocks        # host array: the library copies it into the kernel's argument segment
        # the kernel carries at most twelve blocks in its argument segment: a deeper encoder runs as several launches, each handing the
        # next one its residual stream through the x buffer of its last block
        for s0 in range(0, self.depth, CHAIN_MAX_DEPTH):
            n = min(CHAIN_MAX_DEPTH, self.depth - s0)
            sub = C.cast(C.byref(a.chain_table, s0 * C.sizeof(L.ChainBlock)), C.POINTER(L.ChainBlock))
            rc = L.lib().rgbnm_vit_chain_fwd(C.byref(a.cfg), sub, n, a.xbuf(s0).data_ptr(), L.stream())
            if rc == 1 and s0 == 0:
                self._warn_chain_refused("forward")
                if not self._chain_refused:           # the per-operation kernels need the block shadows this step's prep skipped
                    self._chain_refused = True
                    self._prep(a.cdtype)
                return False
            L.check(rc, "vit_chain_fwd")
        return True

    def _chain_backward(self, a, dy):
        """Run the data path of every block's backward as one launch (rgbnm_vit_chain_bwd); False = not eligible."""
        if (a.cdtype != torch.bfloat16 or self._chain_idx is None or not a.need_grad
                or not L.lib().rgbnm_get_option(b"bwd_chain")):
            return False
        a.build_chain_bwd(self, dy)
        D = self.depth
        starts = list(range(0, D, CHAIN_MAX_DEPTH))
        for s0 in reversed(starts):             # the last blocks first; a launch's first block (lowest index) leaves the next launch its dy
            n = min(CHAIN_MAX_DEPTH, D - s0)
            sub = C.cast(C.byref(a.chain_bwd_table, s0 * C.sizeof(L.ChainBwdBlock)), C.POINTER(L.ChainBwdBlock))
            rc = L.lib().rgbnm_vit_chain_bwd(C.byref(a.cfg), sub, n, a.dattn_chain.data_ptr(), L.stream())
            if rc == 1 and s0 == starts[-1]:
                self._warn_chain_refused("backward")
                if not self._chain_refused:
                    self._chain_refused = True
                    self._prep(a.cdtype)
                return False
            L.check(rc, "vit_chain_bwd")
        return True

    # ---------------------------------------------------------------- arenas
    def _acquire_arena(self, B, cdtype, need_grad):
        key = (B, cdtype, need_grad)
        pool = self._arenas.setdefault(key, [])
        return pool.pop() if pool else _Arena(self, B, cdtype, need_grad)

    def _release_arena(self, arena):
        pool = self._arenas.setdefault((arena.B, arena.cdtype, arena.need_grad), [])
        if len(pool) < 2:
            pool.append(arena)

    # ---------------------------------------------------------------- forward
    def forward(self, x, cbcr=None):
        """x: Y coefficients (B,1,28,28,8,8); cbcr: (B,2,14,14,8,8); fp32, bf16 or fp16 (reference: plainvit.py:601-611).
        Compute dtype: compute_dtype if set, else the autocast dtype (bf16 or fp16), else fp32.  fp16 runs the per-operation
        path on the generic kernels (the one-launch encoder and the other bf16-tuned kernels are bf16 only)."""
        if cbcr is None:
            raise ValueError("DCT path needs both Y and CbCr tensors")
        lam = None
        if isinstance(x, LazyMixed) or isinstance(cbcr, LazyMixed):
            # a batch RandomMixup_DCT(lazy=True) left un-mixed: the group patch embedding mixes while it loads; every other
            # embedding gets the mixed tensors the ordinary way
            if (isinstance(x, LazyMixed) and isinstance(cbcr, LazyMixed) and x.lam.data_ptr() == cbcr.lam.data_ptr()
                    and self.embed_kind == "group"):
                lam, x, cbcr = x.lam, x.tensor, cbcr.tensor
            else:
                x = x.materialize() if isinstance(x, LazyMixed) else x
                cbcr = cbcr.materialize() if isinstance(cbcr, LazyMixed) else cbcr
        L.require_cuda(x, cbcr)
        if x.dim() != 6 or x.shape[1:] != (1, 28, 28, 8, 8) or cbcr.shape[1:] != (2, 14, 14, 8, 8):
            raise ValueError(f"expected Y (B,1,28,28,8,8) and CbCr (B,2,14,14,8,8), got {tuple(x.shape)} {tuple(cbcr.shape)}")
        if x.dtype != cbcr.dtype:
            raise TypeError("Y and CbCr must share a dtype")
        cdtype = self.compute_dtype
        if cdtype is None:
            cdtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
        if cdtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise NotImplementedError(f"compute dtype {cdtype}: the MI355X path implements fp32, bf16 and fp16")
        drop = bool(self.drop_p and self.training)
        if drop and not self.train_dropout:
            raise NotImplementedError("training with dropout p > 0 runs only with model.train_dropout = True (masks from this "
                                      "library's Philox stream, not torch's); model.eval() runs, where nn.Dropout is the identity")
        self._ensure_flat()
        B = x.shape[0]
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self._named.values())
        if need_grad and self._grad_sync is not None:
            self._grad_sync.begin_step()
        self._prep(cdtype, chains=not drop)
        arena = self._acquire_arena(B, cdtype, need_grad)
        st = _FwdState(self, arena, self._grad_buffer() if need_grad else None)
        st.ln_chain = bool(L.lib().rgbnm_vit_ln_chain(C.byref(arena.cfg))) and not drop
        if drop:
            self._begin_dropout(st)
        named = self._named
        if self.embed_kind == "group":
            h = _PatchEmbedFn.apply(x, cbcr, st, named["patchembed.projection.0.weight"],
                                    named["patchembed.projection.0.bias"], lam)
        elif self.embed_kind == "sep_sub":
            h = _PatchEmbed2Fn.apply(x, cbcr, st, *[named[n] for n in _PE2_NAMES])
        elif self.embed_kind == "sep":
            h = _PatchEmbedSepFn.apply(x, cbcr, st, *[named[n] for n in _PES_NAMES])
        else:
            h = _PatchEmbedConcatFn.apply(x, cbcr, st, *[named[n] for n in _PE3_NAMES])
        if (not drop and self.single_encoder_node and cdtype == torch.bfloat16 and self._chain_idx is not None
                and L.lib().rgbnm_get_option(b"fwd_chain")):
            h = _BlocksFn.apply(h, st, 0, self.depth, *self._all_block_params())
        else:
            for i in range(self.depth):
                h = _BlocksFn.apply(h, st, i, i + 1, *[named[n] for n in self._block_param_order[i]])
        out = _HeadFn.apply(h, st, *[named[n] for n in self._head_param_order])
        if isinstance(out, tuple):
            out, edge = out
            out._rgbnm_grad_edge = edge      # cls_transforms.cross_entropy: the compute-dtype gradient edge of these logits
        return out

    def _begin_dropout(self, st):
        """A fresh 64-bit seed for this forward, drawn on the device from torch's default generator (no host sync; a captured
        graph draws a new one on every replay), owned by the forward's state: the backward regenerates the same masks from it,
        whatever other forwards ran in between.  The latest one is model.last_dropout_seed."""
        a = st.arena
        st.drop_seed = torch.empty(1, device=self._flat.device, dtype=torch.int64).random_(-2 ** 63, None)
        self.last_dropout_seed = st.drop_seed
        a.build_dropout(self)
        dy_m = a.drop_dy.data_ptr() if a.need_grad else None
        dxm_m = a.drop_dxmid.data_ptr() if a.need_grad else None
        st.drop = [L.Dropout(st.drop_seed.data_ptr(), self.drop_p, i, dy_m, dxm_m) for i in range(self.depth)]
