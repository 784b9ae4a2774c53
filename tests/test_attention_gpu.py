"""fp64 parity of every reachable instantiation of csrc/attention.hip, through ops.attention_fwd / ops.attention_bwd only.

  attn_fwd_kernel<T, DH, NKT, HP, DROP, TAIL, NW, NSPLIT>   one or two key groups (online softmax), 4 / 8 / 16 waves
  attn_bwd_kernel<T, DH, HP, DROP, NW>                      two phases, 4 / 12 / 16 waves
  attn_bwd1_kernel<32, 2, 8, DROP, TAIL>                    bf16, paired heads, S <= 128: one wave per (document, head)
  attn_bwd2_kernel<NPW, DROP, TAIL=1>                       bf16, head dim 32, dense S >= 256: one pass, dK / dV summed through LDS

`fwd_dispatch` / `bwd_dispatch` restate launch_fwd / launch_bwd; every case carries, written out, the instantiation it is there for
and asserts that the restatement gives it; the CPU self-check ties the restatement to the switches' defaults in attention.hip and
the Makefile, and the REACHABLE_* lists below to what the restatement can return.

Reference: plain torch on the CPU in float64, from the operands AFTER they were rounded to their storage type (masked keys are removed,
not biased; the backward in closed form):
  s = Q K^T / sqrt(dh),  P = softmax,  Pd = P keep scale,  ctx = Pd V,  lse = logsumexp
  dP = dO V^T,  delta = rowsum(dO ctx),  dS = P (dP keep scale - delta),  dQ = dS K / sqrt(dh),  dK = dS^T Q / sqrt(dh),  dV = Pd^T dO
The backward kernels are isolated from the forward: they are given the storage-rounded REFERENCE ctx and fp32(reference lse); one
composed case per backward kernel feeds the forward kernel's own ctx / lse, its bound widened by the forward's bound pushed through
delta (rowsum |dO| b_ctx) and through exp (b_lse added to the relative error of P).

Bound, per element, built from the kernels' rounding points (never fitted; no term carries a free factor).  u = unit roundoff of the
storage type (2^-8 bf16, 2^-24 fp32 parity mode), e = 2^-24, S = the launch's padded length:
  ds_q   = max_k [(dh + 2) e (|Q| |K|^T)_qk / sqrt(dh) + 2 e |s_qk|]                   score: fp32 MFMA sum, scale2 constant, fmaf
  rho_q  = 2 ds_q + (S + 8) e   (backward: + 2 e |lse_q|, lse times log2e)              relative error of a probability
  |d ctx| <= u |ctx| + (u + rho_q + S e) (Pd |V|) + 1e-7
  |d dV|  <= u |dV| + ((u + rho) Pd)^T |dO| + S e Pd^T |dO| + 1e-7
  e_dS   = (u + rho) P (|dP keep scale| + |delta|) + P ((dh + 2) e |dO| |V|^T keep scale + (u + dh e) rowsum |dO ctx|)
  |d dQ|  <= e_dS |K| / sqrt(dh) + u |dQ| + S e |dS| |K| / sqrt(dh)        (dK: transposed, with |Q|)
  |d lse| <= ds_q + (S + 2) e + e sum_k P_k |s_k - max s| + 3 e log S + 2 e |max s| + e |lse|
    the terms: the sum of S terms in fp32 (S e); v_exp_f32 (2 e = 1 ulp relative on every term); the fp32 subtraction under the
    exponential; v_log_f32 (1 ulp of log2 l) and the multiplication by ln 2, with 0 <= log l <= log S; max * ln 2 (constant and
    product); the final add.  The kernel guides give no accuracy figure for v_exp_f32 / v_log_f32: 1 ulp is the figure of AMD's
    instruction set reference ("V_EXP_F32 / V_LOG_F32: 1 ULP accuracy, denormals are flushed").
  The dropped probability matrix read out of the forward (case d) is a CONTEXT row: it carries the store rounding of
  attention.hip:431 (`store4<T>(ctx ..., oacc[dt] * inv)`) as well, which in the two-group kernel follows the rounding of the
  un-normalised probability: (2 u + rho_q + S e) Pd + 2^-126 -- the ctx bound above with |V| = identity and the flush threshold of
  v_exp_f32 in place of 1e-7.
  Operands whose dh-sums are exact in fp32 (case f) drop the two (dh + 2) e terms.

The CPU self-check runs an fp32 emulation of the kernels' rounding points (P rounded to the storage type before PV, dS before its
products, one and two key groups) through the same comparator: every ratio below 1 (worst 0.90 ctx, 0.83 dV), and seven deliberately
wrong variants of it above 1 at every dropout shape of case (a) (the weakest: u = 2^-9 in the bound, 1.61).  On the MI355X the kernels
measure at most 0.91 (ctx) / 0.83 (dV) / 0.72 (dQ) / 0.59 (dK) / 0.08 (lse) of the bound, the dropped probabilities 0.96 (DESIGN
section 4 has the figures per kernel template).  Rows of one case mix score scales 1 / 4 / 16 (queries of row position 0 / 1 / 2 mod 3): unit-scale rows
cancel and sit far inside any bound; the peaked rows of a trained model are where the bound is within a factor of two.

Masked rows: a document with no attended key gives exact zeros in ctx and dqkv; dK / dV rows of masked keys are exact zeros; query
rows of padding positions are ordinary rows (their keys are the document's attended keys) and are checked like any other.
"""
import functools
import math
import os
import re
import zlib

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opensearch-sparse-model-tuning-sample_amd", "csrc")
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
U = {"bf16": 2.0 ** -8, "fp32": 2.0 ** -24}
E = 2.0 ** -24
FLUSH = 2.0 ** -126
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
P_DROP, T_DROP = 0.1, 26                  # make_drop: t = (uint32)(p * 256 + 0.5), scale = 256 / (256 - t)
SEED, SITE = 5, 9
LDS_MAX = 160 * 1024
# the switches of attention.hip this file's dispatch table assumes (the CPU self-check reads the file)
SWITCHES = {"ATTN_SKIP": 1, "ATTN_BWD2": 1, "ATTN_BWD2_S128": 0, "ATTN_BWD2_MIN_S": 256, "ATTN_FWD_SPLIT": 1, "ATTN_BWD_NW_LONG": 16}


# ------------------------------------------------------------------ dispatch, restated
def _rs(dt, width):
    """Lay<T, width>::RS: 128-byte bf16 rows are swizzled, everything else is padded by 16 bytes"""
    size = 2 if dt == "bf16" else 4
    return 128 if (dt == "bf16" and width * size == 128) else width * size + 16


def fwd_dispatch(dt, dh, A, S, ragged, drop):
    """launch_fwd: ("fwd", T, DH, NKT, HP, DROP, TAIL, NW, NSPLIT), or None where SM_REQUIRE(lds <= LDS_MAX) refuses the shape"""
    assert S % 32 == 0 and 32 <= S <= 512 and dh in (32, 64)
    bf = dt == "bf16"
    nkt = 8 if S <= 128 else 16 if S <= 256 else 32
    hp = 2 if (bf and dh == 32 and A % 2 == 0) else 1
    nsp = 2 if (SWITCHES["ATTN_FWD_SPLIT"] and bf and nkt >= 32) else 1
    nw = 16 if nsp > 1 else 8 if (bf and nkt >= 16) else 4
    if 2 * S * _rs(dt, hp * dh) + 4 * S > LDS_MAX:
        return None
    return ("fwd", dt, dh, nkt, hp, int(bool(drop)), int(bool(SWITCHES["ATTN_SKIP"]) and not ragged), nw, nsp)


def bwd_dispatch(dt, dh, A, S, ragged, drop):
    """launch_bwd: ("bwd1", DH, HP, NQT, DROP, TAIL) | ("bwd2", NPW, DROP, TAIL, NW) | ("bwd", T, DH, HP, DROP, NW) | None"""
    bf, d = dt == "bf16", int(bool(drop))
    tail = int(bool(SWITCHES["ATTN_SKIP"]) and not ragged)
    pair = bf and dh == 32 and A % 2 == 0
    if bf and dh == 32:
        if SWITCHES["ATTN_BWD2_S128"] and 64 < S <= 128:
            return ("bwd2", 1, d, tail, 4)
        if S <= 128 and pair:
            return ("bwd1", 32, 2, 8, d, tail)
        if SWITCHES["ATTN_BWD2"] and not ragged and SWITCHES["ATTN_BWD2_MIN_S"] <= S <= 512:
            return ("bwd2", 1 if S <= 256 else 2, d, tail, 8)
    hp = 2 if pair else 1
    if 2 * S * _rs(dt, hp * dh) + hp * 8 * S + S > LDS_MAX:
        return None
    nw = (SWITCHES["ATTN_BWD_NW_LONG"] if pair else 12) if (bf and S > 128) else 4
    return ("bwd", dt, dh, hp, d, nw)


# every instantiation a shape accepted by check_shape can reach (DROP and TAIL / layout multiply each row by the flags named)
#   forward, x DROP 0 / 1 x TAIL 0 (ragged) / 1 (dense): 15 rows, 60 instantiations
_FWD_ROWS = [("bf16", 32, 8, 2, 4, 1), ("bf16", 32, 16, 2, 8, 1), ("bf16", 32, 32, 2, 16, 2),     # paired heads (even A)
             ("bf16", 32, 8, 1, 4, 1), ("bf16", 32, 16, 1, 8, 1), ("bf16", 32, 32, 1, 16, 2),     # odd A
             ("bf16", 64, 8, 1, 4, 1), ("bf16", 64, 16, 1, 8, 1), ("bf16", 64, 32, 1, 16, 2),
             ("fp32", 32, 8, 1, 4, 1), ("fp32", 32, 16, 1, 4, 1), ("fp32", 32, 32, 1, 4, 1),
             ("fp32", 64, 8, 1, 4, 1), ("fp32", 64, 16, 1, 4, 1), ("fp32", 64, 32, 1, 4, 1)]      # the last: S = 288 alone fits the LDS
REACHABLE_FWD = {("fwd", dt, dh, nkt, hp, d, t, nw, nsp) for dt, dh, nkt, hp, nw, nsp in _FWD_ROWS for d in (0, 1) for t in (0, 1)}
#   backward: 22 instantiations.  attn_bwd2_kernel is only launched on the dense layout (TAIL = 1).  attn_bwd_kernel<bf16, 32, 2, *, 4>
#   (paired heads, S <= 128) is instantiated by launch_bwd and UNREACHABLE: attn_bwd1_kernel takes every such shape first.
REACHABLE_BWD = ({("bwd1", 32, 2, 8, d, t) for d in (0, 1) for t in (0, 1)}
                 | {("bwd2", npw, d, 1, 8) for npw in (1, 2) for d in (0, 1)}
                 | {("bwd", "bf16", 32, 2, d, 16) for d in (0, 1)}                                  # paired, ragged S > 128 or dense 129-255
                 | {("bwd", "bf16", dh, 1, d, nw) for dh in (32, 64) for d in (0, 1) for nw in (4, 12)}
                 | {("bwd", "fp32", dh, 1, d, 4) for dh in (32, 64) for d in (0, 1)})
UNREACHABLE_BWD = {("bwd", "bf16", 32, 2, d, 4) for d in (0, 1)}


def enumerate_reachable():
    f, b = set(), set()
    for dt in DTYPES:
        for dh in (32, 64):
            for A in (1, 2, 3, 4, 12):
                for S in range(32, 513, 32):
                    for ragged in (False, True):
                        for drop in (False, True):
                            kf, kb = fwd_dispatch(dt, dh, A, S, ragged, drop), bwd_dispatch(dt, dh, A, S, ragged, drop)
                            assert (kf is None) == (kb is None) or dt == "fp32", (dt, dh, A, S)
                            f |= {kf} - {None}
                            b |= {kb} - {None}
    return f, b


# ------------------------------------------------------------------ cases
# (a): per (type, head dim, layout): (A, S, forward "NKT/HP/NW/NSPLIT", backward) -- the instantiation the row is there for, DROP and
# TAIL following the case's dropout and layout.  Backward: "b1" attn_bwd1_kernel, "b2<NPW>" attn_bwd2_kernel, "2p/HP/NW" the two-phase
# kernel.  Dense documents: one fully attended, one with a prefix of S - 13 keys; ragged: documents of 16 rows, of S rows, of an odd
# number of 16-row tiles ending off the boundary, and of 5 tokens.
A_SHAPES = {
    ("bf16", 32, "dense"): [(2, 32, "8/2/4/1", "b1"), (4, 96, "8/2/4/1", "b1"), (2, 128, "8/2/4/1", "b1"),
                            (4, 160, "16/2/8/1", "2p/2/16"), (2, 224, "16/2/8/1", "2p/2/16"), (2, 256, "16/2/8/1", "b2<1>"),
                            (4, 288, "32/2/16/2", "b2<2>"), (2, 384, "32/2/16/2", "b2<2>"), (4, 480, "32/2/16/2", "b2<2>"),
                            (2, 512, "32/2/16/2", "b2<2>"),
                            (3, 96, "8/1/4/1", "2p/1/4"), (3, 160, "16/1/8/1", "2p/1/12"), (3, 256, "16/1/8/1", "b2<1>"),
                            (3, 384, "32/1/16/2", "b2<2>"), (3, 512, "32/1/16/2", "b2<2>")],
    ("bf16", 32, "ragged"): [(2, 128, "8/2/4/1", "b1"), (4, 256, "16/2/8/1", "2p/2/16"), (2, 512, "32/2/16/2", "2p/2/16"),
                             (3, 96, "8/1/4/1", "2p/1/4"), (3, 224, "16/1/8/1", "2p/1/12"), (3, 480, "32/1/16/2", "2p/1/12")],
    ("bf16", 64, "dense"): [(2, 32, "8/1/4/1", "2p/1/4"), (3, 128, "8/1/4/1", "2p/1/4"), (2, 160, "16/1/8/1", "2p/1/12"),
                            (3, 256, "16/1/8/1", "2p/1/12"), (2, 288, "32/1/16/2", "2p/1/12"), (3, 384, "32/1/16/2", "2p/1/12"),
                            (2, 480, "32/1/16/2", "2p/1/12"), (3, 512, "32/1/16/2", "2p/1/12")],
    ("bf16", 64, "ragged"): [(3, 128, "8/1/4/1", "2p/1/4"), (2, 256, "16/1/8/1", "2p/1/12"), (3, 512, "32/1/16/2", "2p/1/12")],
    ("fp32", 32, "dense"): [(2, 96, "8/1/4/1", "2p/1/4"), (3, 128, "8/1/4/1", "2p/1/4"), (2, 224, "16/1/4/1", "2p/1/4"),
                            (3, 256, "16/1/4/1", "2p/1/4"), (2, 384, "32/1/4/1", "2p/1/4"), (3, 512, "32/1/4/1", "2p/1/4")],
    ("fp32", 32, "ragged"): [(2, 128, "8/1/4/1", "2p/1/4"), (3, 256, "16/1/4/1", "2p/1/4"), (2, 480, "32/1/4/1", "2p/1/4")],
    ("fp32", 64, "dense"): [(2, 96, "8/1/4/1", "2p/1/4"), (3, 160, "16/1/4/1", "2p/1/4"), (2, 256, "16/1/4/1", "2p/1/4"),
                            (3, 288, "32/1/4/1", "2p/1/4")],
    ("fp32", 64, "ragged"): [(2, 128, "8/1/4/1", "2p/1/4"), (3, 256, "16/1/4/1", "2p/1/4"), (2, 288, "32/1/4/1", "2p/1/4")],
}


def named_fwd(dt, dh, layout, drop, name):
    nkt, hp, nw, nsp = (int(x) for x in name.split("/"))
    return ("fwd", dt, dh, nkt, hp, int(bool(drop)), int(layout == "dense"), nw, nsp)


def named_bwd(dt, dh, layout, drop, name):
    d, tail = int(bool(drop)), int(layout == "dense")
    if name == "b1":
        return ("bwd1", 32, 2, 8, d, tail)
    if name.startswith("b2<"):
        return ("bwd2", int(name[3]), d, tail, 8)
    _, hp, nw = name.split("/")
    return ("bwd", dt, dh, int(hp), d, int(nw))


A_CASES = [(dt, dh, layout, A, S, drop, fk, bk) for (dt, dh, layout), rows in A_SHAPES.items() for A, S, fk, bk in rows for drop in (0, 1)]


def _id(c):
    dt, dh, layout, A, S, drop = c[:6]
    return f"{dt}-dh{dh}-A{A}-S{S}-{layout}{'-drop' if drop else ''}"


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


class Case:
    """one launch: rows of every document, key mask, operands in the storage type"""

    def __init__(self, dt, dh, A, S, masks=None, lens=None, drop=False, kind="mixed", seed=0, exact=False):
        self.dt, self.dtype, self.dh, self.A, self.S, self.drop, self.exact = dt, DTYPES[dt], dh, A, S, bool(drop), exact
        self.H, self.u = A * dh, U[dt]
        self.ragged = lens is not None
        if self.ragged:                                    # documents padded to 16 rows, packed; keys pos < len attended
            n = [(x + 15) // 16 * 16 for x in lens]
            assert max(n) <= S
            masks = [torch.arange(k) < x for k, x in zip(n, lens)]
        else:
            n = [S] * len(masks)
        self.masks = [m.bool() for m in masks]
        self.B = len(n)
        self.r0 = [int(x) for x in np.cumsum([0] + n[:-1])]
        self.n, self.rows = n, int(sum(n))
        self.pos = torch.cat([torch.arange(k) for k in n])
        self.keymask = torch.cat(self.masks).to(torch.uint8)
        g = torch.Generator().manual_seed(seed)
        H = self.H
        if exact:   # (f) Q in {-2 .. 2} / 4, K, V, dO in {-2 .. 2}: every dh-product and its sum is exact in fp32 (and in bf16 storage)
            r = lambda *s: torch.randint(-2, 3, s, generator=g).float()
            qkv = torch.cat([r(self.rows, H) / 4, r(self.rows, H), r(self.rows, H)], 1)
            dO = r(self.rows, H)
        else:
            qkv = torch.randn(self.rows, 3 * H, generator=g)
            dO = torch.randn(self.rows, H, generator=g)
            if kind == "mixed":     # score scale 1 / 4 / 16 by row position
                qkv[:, :H] *= torch.tensor([1.0, 4.0, 16.0])[self.pos % 3][:, None]
            elif kind == "peaked":  # 16 x the unit scale on every row
                qkv[:, :H] *= 4.0
                qkv[:, H:2 * H] *= 4.0
            elif kind in ("second_high", "first_high"):  # keys of one group 40 above the other's: s = noise + a b_k / sqrt(dh)
                a = math.sqrt(40 * math.sqrt(dh))
                qkv[:, 0:H:dh] = a
                hi = self.pos >= 256 if kind == "second_high" else self.pos < 256
                qkv[:, H:2 * H:dh] = torch.where(hi, a, 0.0)[:, None]
        self.qkv, self.dO = qkv.to(self.dtype), dO.to(self.dtype)
        if exact:
            assert torch.equal(self.qkv.float(), qkv) and torch.equal(self.dO.float(), dO)

    @property
    def scale(self):
        return 256.0 / (256 - T_DROP) if self.drop else 1.0

    def heads(self, x, b, part=0, width=1):
        """[A, n, dh] float64 view of document b's rows of x ([rows, width * H]; part selects Q / K / V)"""
        s = x[self.r0[b]:self.r0[b] + self.n[b], part * self.H:(part + 1) * self.H]
        return s.reshape(self.n[b], self.A, self.dh).permute(1, 0, 2).double()

    def device_rag(self, ops):
        if not self.ragged:
            return None
        i32 = lambda a: torch.tensor(a, dtype=torch.int32).cuda()
        blk_doc = [b for b in range(self.B) for _ in range(self.n[b] // 16)]
        return ops.Ragged(i32(self.r0 + [self.rows]), i32(blk_doc), self.pos.int().cuda(), self.rows, self.B, self.S)


def a_lens(S):
    """ragged documents of case (a): 16 rows, full length, an odd number of tiles ending off the 16-row boundary, 5 tokens"""
    odd = (S // 16 // 2) | 1
    return [16, S, 16 * odd - 7, 5]


def a_masks(S):
    return [torch.ones(S, dtype=torch.bool), torch.arange(S) < S - 13]


@functools.lru_cache(maxsize=None)
def make_a_case(dt, dh, layout, A, S, drop, exact=False):
    seed = _seed("a", dt, dh, layout, A, S, exact)   # (the same operands with and without dropout)
    if layout == "ragged":
        return Case(dt, dh, A, S, lens=a_lens(S), drop=drop, seed=seed, exact=exact)
    return Case(dt, dh, A, S, masks=a_masks(S), drop=drop, seed=seed, exact=exact)


# ------------------------------------------------------------------ float64 reference and bound
class Ref:
    pass


def _softmax_parts(Q, K, m, dh, exact):
    s = Q @ K.transpose(-1, -2) / math.sqrt(dh)
    absqk = Q.abs() @ K.abs().transpose(-1, -2) / math.sqrt(dh)
    ds_el = 2 * E * s.abs() + (0 if exact else (dh + 2) * E * absqk)
    ds = ds_el.masked_fill(~m, 0).max(-1).values
    sm = s.masked_fill(~m, -float("inf"))
    mx = sm.max(-1).values
    lse = torch.logsumexp(sm, -1)
    P = torch.exp(sm - lse[..., None])
    return s, sm, mx, lse, P, ds


def reference(case, keep=None, u=None, own_fwd=None, backward=True, pd_read=None):
    """fp64 reference and per-element bounds in the launch's row layout.  keep: per document [A, n, n] 0 / 1 (None: no dropout).
    own_fwd: the backward kernel is given the forward KERNEL's ctx / lse (composed case): the backward bound is widened by the
    forward's bound, b_ctx through delta and b_lse through exp.  pd_read: the dropped probabilities read out of the forward, checked
    here element by element (returns the worst ratio in r.pd_ratio)."""
    u = case.u if u is None else u
    dh, A, S, H, c = case.dh, case.A, case.S, case.H, case.scale
    r = Ref()
    r.ctx, r.b_ctx = torch.zeros(case.rows, H, dtype=torch.float64), torch.zeros(case.rows, H, dtype=torch.float64)
    r.lse, r.b_lse = torch.full((case.B, A, S), -float("inf"), dtype=torch.float64), torch.zeros(case.B, A, S, dtype=torch.float64)
    r.lse_valid = torch.zeros(case.B, A, S, dtype=torch.bool)
    r.dqkv, r.b_dqkv = torch.zeros(case.rows, 3 * H, dtype=torch.float64), torch.zeros(case.rows, 3 * H, dtype=torch.float64)
    r.zero_rows = torch.zeros(case.rows, dtype=torch.bool)     # documents without an attended key: exact zeros everywhere
    r.zero_keys = ~case.keymask.bool()                         # masked keys: exact zeros in dK / dV
    r.pd_ratio = 0.0
    back = lambda x: x.permute(1, 0, 2).reshape(x.shape[1], H)
    for b in range(case.B):
        n, m, sl = case.n[b], case.masks[b], slice(case.r0[b], case.r0[b] + case.n[b])
        if not m.any():
            r.zero_rows[sl] = True
            continue
        Q, K, V = (case.heads(case.qkv, b, i) for i in range(3))
        s, sm, mx, lse, P, ds = _softmax_parts(Q, K, m, dh, case.exact)
        kc = (keep[b].double() * c) if keep is not None else torch.ones_like(P)
        Pd = P * kc
        rho = 2 * ds + (S + 8) * E
        ctx = Pd @ V
        b_ctx = u * ctx.abs() + (u + rho + S * E)[..., None] * (Pd @ V.abs()) + 1e-7
        spread = (P * (sm - mx[..., None]).abs().masked_fill(~m, 0)).sum(-1)
        b_lse = ds + (S + 2) * E + E * spread + 3 * E * math.log(S) + 2 * E * mx.abs() + E * lse.abs()
        r.ctx[sl], r.b_ctx[sl] = back(ctx), back(b_ctx)
        r.lse[b, :, :n], r.b_lse[b, :, :n], r.lse_valid[b, :, :n] = lse, b_lse, True
        if pd_read is not None:
            bound = (2 * u + rho + S * E)[..., None] * (P * c) + FLUSH
            r.pd_ratio = max(r.pd_ratio, float(((pd_read[b].double() - Pd).abs() / bound).max()))
        if not backward:
            continue
        dO = case.heads(case.dO, b)
        x_rho = x_delta = 0.0
        if own_fwd is not None:   # what the kernel is given: its own forward's outputs
            x_rho, x_delta = b_lse, (dO.abs() * b_ctx).sum(-1)   # (the reference stays the exact one; the bound carries the forward's error)
        dP = dO @ V.transpose(-1, -2)
        dPk = dP * kc
        delta, adelta = (dO * ctx).sum(-1), (dO * ctx).abs().sum(-1)
        dS = P * (dPk - delta[..., None])
        rb = rho + 2 * E * lse.abs() + x_rho
        prod = 0 if case.exact else (dh + 2) * E * (dO.abs() @ V.abs().transpose(-1, -2)) * kc
        e_dS = (u + rb)[..., None] * P * (dPk.abs() + delta.abs()[..., None]) + P * (prod + ((u + dh * E) * adelta + x_delta)[..., None])
        q = 1 / math.sqrt(dh)
        dQ, dK, dV = dS @ K * q, dS.transpose(-1, -2) @ Q * q, Pd.transpose(-1, -2) @ dO
        b_dQ = e_dS @ K.abs() * q + u * dQ.abs() + S * E * (dS.abs() @ K.abs()) * q
        b_dK = e_dS.transpose(-1, -2) @ Q.abs() * q + u * dK.abs() + S * E * (dS.abs().transpose(-1, -2) @ Q.abs()) * q
        b_dV = u * dV.abs() + ((u + rb)[..., None] * Pd).transpose(-1, -2) @ dO.abs() + S * E * (Pd.transpose(-1, -2) @ dO.abs()) + 1e-7
        r.dqkv[sl] = torch.cat([back(dQ), back(dK), back(dV)], 1)
        r.b_dqkv[sl] = torch.cat([back(b_dQ), back(b_dK), back(b_dV)], 1)
    return r


def bwd_inputs(case, ref):
    """what the isolated backward is given: the reference ctx rounded to the storage type, the reference lse in fp32"""
    return ref.ctx.to(case.dtype), ref.lse.float()


def ratios(case, ref, ctx=None, lse=None, dqkv=None, tag="", exact_zeros=True):
    """the comparator: worst error over bound per output (dict), after the finiteness and exact-zero checks (exact_zeros = False, the
    negative controls: a non-finite element counts as an infinite ratio instead)"""
    out, H = {}, case.H
    live = ~ref.zero_rows
    f64 = lambda x: x.detach().cpu().double() if exact_zeros else torch.nan_to_num(x.detach().cpu().double(), nan=1e300, posinf=1e300, neginf=-1e300)
    if ctx is not None:
        ctx = f64(ctx)
        assert torch.isfinite(ctx).all(), f"{tag}: ctx not finite"
        if exact_zeros:
            assert (ctx[ref.zero_rows] == 0).all(), f"{tag}: ctx of a document without attended keys is not zero"
        out["ctx"] = float(((ctx - ref.ctx).abs() / ref.b_ctx)[live].max())
    if lse is not None:
        lse = f64(lse)
        v = ref.lse_valid
        assert torch.isfinite(lse[v]).all(), f"{tag}: lse not finite"
        out["lse"] = float(((lse - ref.lse).abs()[v] / ref.b_lse[v]).max())
    if dqkv is not None:
        dqkv = f64(dqkv)
        assert torch.isfinite(dqkv).all(), f"{tag}: dqkv not finite"
        if exact_zeros:
            assert (dqkv[ref.zero_rows] == 0).all(), f"{tag}: dqkv of a document without attended keys is not zero"
            assert (dqkv[ref.zero_keys][:, H:] == 0).all(), f"{tag}: dK / dV of a masked key is not zero"
        err = (dqkv - ref.dqkv).abs()
        keys = live & ~ref.zero_keys
        out["dQ"] = float((err[:, :H] / ref.b_dqkv[:, :H])[live].max())
        if keys.any():
            out["dK"] = float((err[:, H:2 * H] / ref.b_dqkv[:, H:2 * H])[keys].max())
            out["dV"] = float((err[:, 2 * H:] / ref.b_dqkv[:, 2 * H:])[keys].max())
    return out


def hold(rat, tag):
    print(f"attn_ratio {tag}: " + " ".join(f"{k}={v:.4f}" for k, v in rat.items()))
    bad = {k: v for k, v in rat.items() if not v <= 1}
    assert not bad, f"{tag}: error over bound {bad}"


# ------------------------------------------------------------------ fp32 emulation of the kernels' rounding points (CPU self-check)
def _rnd(x, dt):
    return x.to(torch.bfloat16).float() if dt == "bf16" else x


def _bug_mask(m, bug):
    if bug == "mask_shift":
        return torch.roll(m, 1)
    if bug == "last_tile":
        m = m.clone()
        m[int(m.nonzero().max()) // 16 * 16:] = False
    return m


def emulate(case, keep=None, ref=None, bug=None):
    """ctx, lse, dqkv as the kernels round: fp32 sums, exp2 in the log2 domain, P (un-normalised in the two-group forward) and dS
    rounded to the storage type before the sequence products, outputs rounded when stored.  The backward takes bwd_inputs(ref)."""
    dt, dh, S, H, c = case.dt, case.dh, case.S, case.H, np.float32(case.scale)
    nsplit = fwd_dispatch(dt, dh, case.A, S, case.ragged, case.drop)[-1]
    scale = np.float32(1 / math.sqrt(dh))
    scale2 = np.float32(scale * np.float32(LOG2E))
    ctx, lse = torch.zeros(case.rows, H), torch.full((case.B, case.A, S), -float("inf"))
    dqkv = torch.zeros(case.rows, 3 * H)
    back = lambda x: x.permute(1, 0, 2).reshape(x.shape[1], H)
    ctx_in, lse_in = bwd_inputs(case, ref)
    for b in range(case.B):
        n, sl = case.n[b], slice(case.r0[b], case.r0[b] + case.n[b])
        if not case.masks[b].any():
            continue
        m = _bug_mask(case.masks[b], bug)
        Q, K, V = (case.heads(case.qkv, b, i).float() for i in range(3))
        dO = case.heads(case.dO, b).float()
        kc = None
        if keep is not None:
            kc = (torch.roll(keep[b], 1, -1) if bug == "keep_shift" else keep[b]).float() * c
        s2 = ((Q @ K.transpose(-1, -2)) * scale2).masked_fill(~m, -float("inf"))
        m_run, l_run, o = torch.full(s2.shape[:2], -1e30), torch.zeros(s2.shape[:2]), torch.zeros_like(Q)
        for a, z in ([(0, n)] if nsplit == 1 or n <= 256 else [(0, 256), (256, n)]):
            g = s2[..., a:z]
            mx = torch.maximum(g.max(-1).values, m_run)
            e = torch.exp2(g - mx[..., None])
            sm = e.sum(-1)
            alpha = torch.ones_like(mx) if bug == "no_alpha" else torch.exp2(m_run - mx)
            l_run, m_run = l_run * alpha + sm, mx
            p = e * torch.where(sm > 0, 1 / sm, torch.zeros_like(sm))[..., None] if nsplit == 1 else e
            if kc is not None:
                p = p * kc[..., a:z]
            o = o * alpha[..., None] + _rnd(p, dt) @ V[:, a:z]
        if nsplit > 1:
            o = o * torch.where(l_run > 0, 1 / l_run, torch.zeros_like(l_run))[..., None]
        ctx[sl], lse[b, :, :n] = back(_rnd(o, dt)), m_run * np.float32(LN2) + torch.log(l_run)
        # backward, isolated
        ci, lq = case.heads(ctx_in.float(), b).float(), lse_in[b, :, :n] * np.float32(LOG2E)
        pv = torch.exp2((Q @ K.transpose(-1, -2)) * scale2 - lq[..., None]).masked_fill(~m, 0)
        delta = (dO * ci).sum(-1)
        if bug == "delta_noscale":
            delta = delta / c
        one = torch.ones_like(pv)
        kcb = one if kc is None else kc
        ds = _rnd(pv * ((dO @ V.transpose(-1, -2)) * kcb - delta[..., None]), dt)
        pd = _rnd(pv * kcb, dt)
        dQ = _rnd((ds @ K) * scale, dt)
        dK = _rnd((ds.transpose(-1, -2) @ Q) * (np.float32(1) if bug == "dk_noscale" else scale), dt)
        dV = _rnd(pd.transpose(-1, -2) @ dO, dt)
        dqkv[sl] = torch.cat([back(dQ), back(dK), back(dV)], 1)
    return ctx, lse, dqkv


def synthetic_keep(case, seed=1):
    """a Bernoulli keep mask at the kernels' quantised rate (the CPU self-check has no kernel to read one from)"""
    if not case.drop:
        return None
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (case.A, n, n), generator=g) >= T_DROP for n in case.n]


# ------------------------------------------------------------------ CPU: the test's own machinery
def _autograd_check(case, keep):
    ref = reference(case, keep)
    x = case.qkv.double().requires_grad_(True)
    c, H = case.scale, case.H
    ctxs = []
    for b in range(case.B):
        n, m = case.n[b], case.masks[b]
        if not m.any():
            ctxs.append(torch.zeros(n, H, dtype=torch.float64))
            continue
        Q, K, V = (x[case.r0[b]:case.r0[b] + n, i * H:(i + 1) * H].reshape(n, case.A, case.dh).permute(1, 0, 2) for i in range(3))
        s = (Q @ K.transpose(-1, -2) / math.sqrt(case.dh))[..., m]       # masked keys removed
        P = torch.softmax(s, -1)
        if keep is not None:
            P = P * keep[b][..., m].double() * c
        ctxs.append((P @ V[:, m]).permute(1, 0, 2).reshape(n, H))
        assert float((torch.logsumexp(s, -1).detach() - ref.lse[b, :, :n]).abs().max()) <= 1e-12
    ctx = torch.cat(ctxs)
    (ctx * case.dO.double()).sum().backward()
    tol = 1e-12 * max(1.0, float(x.grad.abs().max()))
    assert float((ctx.detach() - ref.ctx).abs().max()) <= 1e-12 and float((x.grad - ref.dqkv).abs().max()) <= tol


NEGATIVE = ("mask_shift", "keep_shift", "no_alpha", "last_tile", "dk_noscale", "delta_noscale", "half_u")


def test_reference_bound_comparator_and_dispatch_table():
    # --- dispatch: the switches' defaults, no -DATTN_ in the build, the reachable set, every reachable instantiation covered by (a)
    src = open(os.path.join(CSRC, "attention.hip")).read()
    for name, value in SWITCHES.items():
        got = re.search(r"#ifndef %s\n#define %s (\d+)" % (name, name), src)
        assert got is not None and int(got.group(1)) == value, f"{name}: attention.hip defaults to {got and got.group(1)}, the table assumes {value}"
    assert "-DATTN_" not in open(os.path.join(CSRC, "Makefile")).read()
    assert "S % 32 == 0 && S >= 32 && S <= 512" in src and "constexpr size_t LDS_MAX = 160 * 1024;" in src
    assert "uint32_t t = (uint32_t)(s->p * 256.0f + 0.5f);" in open(os.path.join(CSRC, "common.h")).read() and int(P_DROP * 256 + 0.5) == T_DROP
    f, b = enumerate_reachable()
    assert f == REACHABLE_FWD and len(f) == 60, sorted(f ^ REACHABLE_FWD)
    assert b == REACHABLE_BWD and len(b) == 22 and not (b & UNREACHABLE_BWD), sorted(b ^ REACHABLE_BWD)
    cov_f, cov_b = set(), set()
    for dt, dh, layout, A, S, drop, fk, bk in A_CASES:
        kf, kb = named_fwd(dt, dh, layout, drop, fk), named_bwd(dt, dh, layout, drop, bk)
        assert fwd_dispatch(dt, dh, A, S, layout == "ragged", drop) == kf, (dt, dh, layout, A, S, drop)
        assert bwd_dispatch(dt, dh, A, S, layout == "ragged", drop) == kb, (dt, dh, layout, A, S, drop)
        cov_f.add(kf)
        cov_b.add(kb)
    assert cov_f == REACHABLE_FWD and cov_b == REACHABLE_BWD, (sorted(REACHABLE_FWD - cov_f), sorted(REACHABLE_BWD - cov_b))
    assert {c[4] for c in A_CASES} == {32, 96, 128, 160, 224, 256, 288, 384, 480, 512}
    for S in (96, 128, 224, 256, 288, 480, 512):   # ragged documents: 16 rows, full, an odd tile count off the boundary
        n16 = [(x + 15) // 16 for x in a_lens(S)]
        assert n16[0] == 1 and a_lens(S)[1] == S and n16[2] % 2 == 1 and a_lens(S)[2] % 16 and 16 * n16[2] <= S
    # --- the composed and the determinism cases reach every backward kernel; determinism: attn_bwd2 at 256 / 384 / 512, the 16-wave forward
    assert {bwd_family(c) for c in COMPOSED} == BWD_FAMILIES and {bwd_family(c) for c in DETERMINISM} == BWD_FAMILIES
    assert {c[4] for c in DETERMINISM if bwd_family(c).startswith("b2")} == {256, 384, 512}
    assert any(fwd_dispatch(c[0], c[1], c[3], c[4], c[2] == "ragged", c[5])[7] == 16 for c in DETERMINISM)
    # --- the reference against autograd through the removed keys (small shapes, both layouts, with and without a keep mask)
    for dt, dh, A, kw in (("fp32", 32, 3, dict(masks=[torch.arange(32) < 20, torch.arange(32) % 3 > 0, torch.zeros(32, dtype=torch.bool)])),
                          ("fp32", 64, 2, dict(lens=[16, 27, 5]))):
        for drop in (0, 1):
            case = Case(dt, dh, A, 32, drop=drop, seed=3, **kw)
            _autograd_check(case, synthetic_keep(case))
    # --- the bound against the emulation, and the comparator against wrong variants of it, at every shape of (a) (dropout on: the
    # superset of rounding points; the dropout-off twins of four shapes as well)
    worst, missed = {}, []
    todo = [c for c in A_CASES if c[5]] + [c for c in A_CASES if not c[5] and c[4] in (96, 512)]
    for dt, dh, layout, A, S, drop, fk, bk in todo:
        case = make_a_case(dt, dh, layout, A, S, drop)
        keep = synthetic_keep(case)
        ref = reference(case, keep)
        rat = ratios(case, ref, *emulate(case, keep, ref))
        for k, v in rat.items():
            key = (dt, "fwd2" if fk.endswith("/2") else "fwd1") if k in ("ctx", "lse") else (dt, "bwd")
            worst[key + (k,)] = max(worst.get(key + (k,), 0.0), v)
        assert max(rat.values()) <= 1, (_id((dt, dh, layout, A, S, drop)), rat)
        if not drop:
            continue
        for bug in NEGATIVE:
            if (bug == "no_alpha" and not fk.endswith("/2")) or (bug == "half_u" and dt != "bf16"):
                continue   # no second key group to rescale; u = 2^-9 is a statement about bf16
            if bug == "half_u":
                bad = ratios(case, reference(case, keep, u=case.u / 2), *emulate(case, keep, ref))
            else:
                bad = ratios(case, ref, *emulate(case, keep, ref, bug=bug), exact_zeros=False)
            worst[("neg", bug)] = min(worst.get(("neg", bug), float("inf")), max(bad.values()))
            if not max(bad.values()) > 1:
                missed.append((_id((dt, dh, layout, A, S, drop)), bug, max(bad.values())))
    for k in sorted(worst, key=str):
        print("attn_emulation", *k, f"{worst[k]:.4f}")
    assert not missed, missed


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sparse_hip import ops as _ops
    from sparse_hip import lib
    lib.load()
    return _ops


def _drop(case, seed=SEED, site=SITE):
    from sparse_hip import lib
    return lib.dropout(P_DROP, seed, site) if case.drop else None


def run_fwd(ops, case, qkv=None, **kw):
    ctx, lse = ops.attention_fwd((case.qkv if qkv is None else qkv).cuda(), case.keymask.cuda(), case.B, case.S, case.A, _drop(case, **kw),
                                 case.device_rag(ops))
    torch.cuda.synchronize()
    return ctx, lse


def run_bwd(ops, case, ctx, lse):
    dqkv = ops.attention_bwd(case.qkv.cuda(), case.keymask.cuda(), ctx.cuda(), case.dO.cuda(), lse.cuda(), case.B, case.S, case.A, _drop(case),
                             case.device_rag(ops))
    torch.cuda.synchronize()
    return dqkv


def read_pd(ops, case, value=1.0, **kw):
    """the dropped probability matrix Pd[b][h, q, k] out of the forward kernel: the real Q and K, V[k, j] = value where k == c dh + j
    (row position k inside its document), one launch per block c of dh keys: ctx[q, h dh + j] = value * Pd[q, c dh + j]"""
    dh, H, A = case.dh, case.H, case.A
    pd = [torch.zeros(A, n, n) for n in case.n]
    for c in range(-(-max(case.n) // dh)):
        qkv = case.qkv.clone()
        v = torch.zeros(case.rows, A, dh)
        inb = (case.pos >= c * dh) & (case.pos < (c + 1) * dh)
        v[inb, :, (case.pos[inb] - c * dh)] = value
        qkv[:, 2 * H:] = v.reshape(case.rows, H).to(case.dtype)
        ctx = run_fwd(ops, case, qkv, **kw)[0].float().cpu() / value
        for b, n in enumerate(case.n):
            w = min(dh, n - c * dh)   # (a document of 16 rows ends inside a block of 32)
            if w > 0:
                pd[b][:, :, c * dh:c * dh + w] = ctx[case.r0[b]:case.r0[b] + n].reshape(n, A, dh).permute(1, 0, 2)[..., :w]
    return pd


def read_keep(ops, case, **kw):
    pd = read_pd(ops, case, **kw)
    return pd, [p > 0 for p in pd]


def assert_dispatch(case, fwd=None, bwd=None):
    if fwd is not None:
        assert fwd_dispatch(case.dt, case.dh, case.A, case.S, case.ragged, case.drop) == fwd, (fwd, "is not what launch_fwd picks")
    if bwd is not None:
        assert bwd_dispatch(case.dt, case.dh, case.A, case.S, case.ragged, case.drop) == bwd, (bwd, "is not what launch_bwd picks")


def bwd_family(spec):
    """the backward kernel template (with what selects its code path) a case spec is dispatched to"""
    dt, dh, layout, A, S, drop = spec
    k = bwd_dispatch(dt, dh, A, S, layout == "ragged", drop)
    return {"bwd1": lambda: "b1", "bwd2": lambda: f"b2<{k[1]}>", "bwd": lambda: f"2p/{k[1]}/{k[5]}"}[k[0]]()


BWD_FAMILIES = {"b1", "b2<1>", "b2<2>", "2p/bf16/16", "2p/bf16/12", "2p/bf16/4", "2p/fp32/4"}


def kernel_tag(k):
    return {"fwd": lambda: f"attn_fwd<{k[1]},NSPLIT={k[8]}>", "bwd": lambda: f"attn_bwd<{k[1]}>", "bwd1": lambda: "attn_bwd1<bf16>",
            "bwd2": lambda: "attn_bwd2<bf16>"}[k[0]]()


@gpu
@pytest.mark.parametrize("spec", A_CASES, ids=_id)
def test_every_instantiation_against_fp64(ops, spec):
    """(a) one case per reachable forward and backward instantiation (and per length of the issue's list); with dropout the keep mask is
    the one READ OUT of the forward kernel, for the forward's and the backward's reference alike: a backward kernel that regenerates
    another bit fails its bound"""
    dt, dh, layout, A, S, drop, fk, bk = spec
    case = make_a_case(dt, dh, layout, A, S, drop)
    kf, kb = named_fwd(dt, dh, layout, drop, fk), named_bwd(dt, dh, layout, drop, bk)
    assert_dispatch(case, kf, kb)
    pd = keep = None
    if drop:
        pd, keep = read_keep(ops, case)
    ref = reference(case, keep, pd_read=pd)
    if drop:
        print(f"attn_ratio {_id(spec)} {kernel_tag(kf)} Pd={ref.pd_ratio:.4f}")
        assert ref.pd_ratio <= 1, f"dropped probabilities: {ref.pd_ratio:.3f} x the bound"
    ctx, lse = run_fwd(ops, case)
    hold(ratios(case, ref, ctx, lse), f"{_id(spec)} {kernel_tag(kf)}")
    dqkv = run_bwd(ops, case, *bwd_inputs(case, ref))
    hold(ratios(case, ref, dqkv=dqkv), f"{_id(spec)} {kernel_tag(kb)}")


COMPOSED = [("bf16", 32, "dense", 2, 128, 1), ("bf16", 32, "dense", 2, 256, 1), ("bf16", 32, "dense", 4, 480, 1),      # bwd1, bwd2<1>, bwd2<2>
            ("bf16", 32, "ragged", 4, 256, 1), ("bf16", 64, "dense", 3, 384, 1), ("bf16", 32, "dense", 3, 96, 1),      # two-phase 16 / 12 / 4 waves
            ("fp32", 64, "dense", 3, 160, 1), ("fp32", 32, "ragged", 2, 480, 0)]


@gpu
@pytest.mark.parametrize("spec", COMPOSED, ids=_id)
def test_backward_on_the_forward_kernels_own_outputs(ops, spec):
    """the composed path of a training step: the backward kernel reads the ctx / lse the forward kernel wrote; the bound carries the
    forward's bound through delta and exp"""
    case = make_a_case(*spec)
    keep = read_keep(ops, case)[1] if case.drop else None
    ctx, lse = run_fwd(ops, case)
    ref = reference(case, keep, own_fwd=True)
    hold(ratios(case, ref, ctx, lse), f"composed {_id(spec)} fwd")
    lse_in = torch.where(ref.lse_valid, lse.cpu(), torch.zeros(()))
    dqkv = run_bwd(ops, case, ctx, lse_in)
    hold(ratios(case, ref, dqkv=dqkv), f"composed {_id(spec)} {kernel_tag(bwd_dispatch(case.dt, case.dh, case.A, case.S, case.ragged, case.drop))}")


def b_masks(S):
    """(b) the masks of test_attention_dense_layout_skips_only_the_masked_tail at any S, plus documents whose last attended key is the
    first / the last key of a 16-key tile"""
    ar, f = torch.arange(S), S / 128
    hole = (ar < int(96 * f)) & ~((ar >= int(20 * f)) & (ar < int(70 * f)))
    return [ar < S, ar < 16, ar < int(33 * f), hole, ar == S - 1, ar == 0, ar < int(64 * f) + 3, ar < 0,
            ar < S // 2 + 1 - (S // 2) % 16 + 16, ar < (S // 2) // 16 * 16]


@gpu
@pytest.mark.parametrize("S", [160, 384, 480])
@pytest.mark.parametrize("dh,A", [(32, 2), (32, 3), (64, 2)])
def test_dense_masks_at_the_new_lengths(ops, dh, A, S):
    """(b) prefix, hole, only the last key, only the first key, nothing attended; the skipped tail of the forward and of
    attn_bwd1 / attn_bwd2 ends at the last attended key"""
    masks = b_masks(S)
    last = [int(m.nonzero().max()) for m in masks if m.any()]
    assert any(x % 16 == 0 for x in last) and any(x % 16 == 15 for x in last) and not masks[7].any()
    case = Case("bf16", dh, A, S, masks=masks, seed=_seed("b", dh, A, S))
    ref = reference(case)
    assert int(ref.zero_rows.sum()) == S
    ctx, lse = run_fwd(ops, case)
    hold(ratios(case, ref, ctx, lse), f"masks dh{dh}-A{A}-S{S} fwd")
    hold(ratios(case, ref, dqkv=run_bwd(ops, case, *bwd_inputs(case, ref))), f"masks dh{dh}-A{A}-S{S} bwd")


@gpu
@pytest.mark.parametrize("kind", ["second_high", "first_high", "first_masked", "second_masked", "peaked"])
@pytest.mark.parametrize("S", [384, 512])
@pytest.mark.parametrize("dh,A", [(32, 2), (32, 3), (64, 2)])
def test_two_group_online_softmax(ops, dh, A, S, kind):
    """(c) attn_fwd_kernel<.., NSPLIT = 2>: the second key group's maximum 40 above the first's and the reverse (alpha = e^-40 / the
    second group's terms e^-40), one whole group masked, scores 16 x the unit scale"""
    ar = torch.arange(S)
    masks = {"first_masked": [ar >= 256, ar >= 300], "second_masked": [ar < 256, ar < 200]}.get(kind, [ar < S, ar < S - 13])
    case = Case("bf16", dh, A, S, masks=masks, kind=kind if kind in ("second_high", "first_high", "peaked") else "mixed", seed=_seed("c", dh, A, S, kind))
    assert fwd_dispatch("bf16", dh, A, S, False, False) == ("fwd", "bf16", dh, 32, 2 if A % 2 == 0 and dh == 32 else 1, 0, 1, 16, 2)
    ref = reference(case, backward=False)
    if kind in ("second_high", "first_high"):
        Q, K = case.heads(case.qkv, 0, 0), case.heads(case.qkv, 0, 1)
        s = Q @ K.transpose(-1, -2) / math.sqrt(dh)
        gap = s[..., 256:].max(-1).values - s[..., :256].max(-1).values
        assert float(s.abs().max()) < 80, float(s.abs().max())
        assert (gap > 30).all() if kind == "second_high" else (gap < -30).all(), (float(gap.min()), float(gap.max()))
    ctx, lse = run_fwd(ops, case)
    hold(ratios(case, ref, ctx, lse), f"two-group {kind} dh{dh}-A{A}-S{S} attn_fwd<bf16,NSPLIT=2>")


@gpu
def test_dropout_mask_properties(ops):
    """(d) the keep mask itself, read out of the forward: independent of V; different between seeds, sites, heads and documents; the
    same (document, head, query, key) bit in the dense and the ragged layout; drop rate within four binomial standard deviations of
    t / 256 over N = 131072 elements; kept probabilities scaled by 256 / (256 - t) (the element-wise bound of `reference`)"""
    dense = Case("bf16", 32, 4, 128, masks=[torch.ones(128, dtype=torch.bool)] * 2, drop=True, kind="unit", seed=11)  # (unit scale: no probability underflows)
    pd, keep = read_keep(ops, dense)
    ref = reference(dense, keep, pd_read=pd, backward=False)
    print(f"attn_ratio mask-properties Pd={ref.pd_ratio:.4f}")
    assert ref.pd_ratio <= 1    # ... against P keep 256 / (256 - t)
    keep = torch.stack(keep)    # [B, A, S, S]
    N = keep.numel()
    rate, want = 1 - float(keep.double().mean()), T_DROP / 256
    sd = math.sqrt(want * (1 - want) / N)
    print(f"attn_drop_rate {rate:.6f} want {want:.6f} sd {sd:.6f} N {N}")
    assert N >= 65536 and abs(rate - want) <= 4 * sd, (rate, want, sd)
    assert torch.equal(torch.stack(read_keep(ops, dense, value=-3.0)[1]), keep), "the keep mask changes with V"
    for what, other in (("seed", torch.stack(read_keep(ops, dense, seed=SEED + 1)[1])), ("site", torch.stack(read_keep(ops, dense, site=SITE + 1)[1]))):
        same = float((other == keep).double().mean())
        assert abs(same - (want ** 2 + (1 - want) ** 2)) <= 0.01, f"another {what}: {same:.4f} of the bits agree"
    indep = want ** 2 + (1 - want) ** 2
    assert abs(float((keep[0] == keep[1]).double().mean()) - indep) <= 0.01, "two documents share their mask"
    for h in range(1, 4):
        assert abs(float((keep[:, 0] == keep[:, h]).double().mean()) - indep) <= 0.01, "two heads share their mask"
    ragged = Case("bf16", 32, 4, 128, lens=[128, 128], drop=True, kind="unit", seed=11)
    assert torch.equal(ragged.qkv, dense.qkv)
    assert torch.equal(torch.stack(read_keep(ops, ragged)[1]), keep), "dense and ragged layout disagree on a keep bit"


DETERMINISM = [("bf16", 32, "dense", 2, 256, 1), ("bf16", 32, "dense", 2, 384, 1), ("bf16", 32, "dense", 2, 512, 1), ("bf16", 32, "dense", 3, 384, 1),
               ("bf16", 32, "dense", 2, 128, 1), ("bf16", 32, "dense", 4, 160, 1), ("bf16", 32, "ragged", 2, 512, 1), ("bf16", 64, "dense", 3, 512, 1),
               ("bf16", 32, "dense", 3, 96, 1), ("fp32", 32, "dense", 2, 224, 1)]


@gpu
@pytest.mark.parametrize("spec", DETERMINISM, ids=_id)
def test_three_launches_are_bit_identical(ops, spec):
    """(e) attn_bwd2_kernel sums dK / dV over eight waves through two LDS parities: a missing barrier shows as run-to-run differences.
    Every backward kernel and the 16-wave forward, three launches on the same inputs"""
    case = make_a_case(*spec)
    ctx0, lse0 = run_fwd(ops, case)
    d0 = run_bwd(ops, case, ctx0, torch.nan_to_num(lse0, nan=0.0, posinf=0.0, neginf=0.0))
    bits = lambda x: x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)
    for _ in range(2):
        ctx, lse = run_fwd(ops, case)
        assert torch.equal(bits(ctx), bits(ctx0)) and torch.equal(bits(lse)[:, :, :min(case.n)], bits(lse0)[:, :, :min(case.n)])
        d = run_bwd(ops, case, ctx0, torch.nan_to_num(lse0, nan=0.0, posinf=0.0, neginf=0.0))
        assert torch.equal(bits(d), bits(d0))


EXACT = [("bf16", 32, "dense", 2, 128, 0), ("bf16", 32, "dense", 2, 256, 1), ("bf16", 32, "dense", 4, 480, 0), ("bf16", 32, "dense", 3, 512, 1),
         ("bf16", 32, "ragged", 2, 512, 0), ("bf16", 32, "ragged", 3, 224, 1), ("bf16", 64, "dense", 2, 288, 0), ("bf16", 64, "ragged", 3, 512, 1),
         ("bf16", 32, "dense", 3, 96, 0), ("fp32", 32, "dense", 3, 512, 0), ("fp32", 64, "dense", 3, 288, 1), ("fp32", 64, "ragged", 2, 128, 0)]


@gpu
@pytest.mark.parametrize("spec", EXACT, ids=_id)
def test_exactly_representable_operands(ops, spec):
    """(f) Q, K, V, dO of small integers (Q over 4): every head-dim product and sum is exact in fp32, the (dh + 2) e terms leave the
    bound and what remains is the rounding of P, dS and the outputs -- a mis-indexed tile cannot hide inside it"""
    case = make_a_case(*spec, exact=True)
    keep = read_keep(ops, case)[1] if case.drop else None
    ref = reference(case, keep)
    ctx, lse = run_fwd(ops, case)
    hold(ratios(case, ref, ctx, lse), f"exact {_id(spec)} {kernel_tag(fwd_dispatch(case.dt, case.dh, case.A, case.S, case.ragged, case.drop))}")
    dqkv = run_bwd(ops, case, *bwd_inputs(case, ref))
    hold(ratios(case, ref, dqkv=dqkv), f"exact {_id(spec)} {kernel_tag(bwd_dispatch(case.dt, case.dh, case.A, case.S, case.ragged, case.drop))}")
