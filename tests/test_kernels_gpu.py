"""GPU parity tests, one per C-ABI kernel family: the HIP kernel (called through ctypes)
against the CPU oracle / a plain torch fp32 restatement on the same seeded inputs.
Tolerances: fp32 storage 1e-3 (north_star "1e-3 fp32"), bf16 storage 1e-2 relative to the
tensor's scale (north_star "1e-2 bf16"), written per test."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sparse_oracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DTYPES = [torch.float32, torch.bfloat16]
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sparse_hip import ops as _ops
    from sparse_hip import lib
    lib.load()
    return _ops


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None and t.is_floating_point():
        t = t.to(dtype)
    return t.cuda().contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def q(x, dtype):
    """round-trip through the storage dtype so the reference sees the same inputs"""
    return x.to(dtype).float()


def close(got, want, tol, what=""):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol} * {scale:.3e}"


# ------------------------------------------------------------------ GEMM NT
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(200, 136, 128), (128, 128, 64), (77, 520, 192), (300, 64, 384),
                                   # large shapes (many row tiles, XCD-aware tile order)
                                   (8200, 384, 384), (8197, 256, 128), (4100, 256, 1536), (6200, 768, 64), (6151, 1152, 384),
                                   (33017, 384, 128),
                                   # N = 384, K >= 1024, one round of 192-row tiles: bf16 takes gemm_nt192_kernel
                                   (6200, 384, 1024), (6151, 384, 1152),
                                   # two column blocks, >= 512 tiles: the same kernel over several rounds (bert-base shapes)
                                   (49200, 768, 1024)])
def test_gemm_nt_plain_and_epilogues(ops, dtype, M, N, K):
    A, B = q(rnd(M, K, seed=1, scale=0.5), dtype), q(rnd(N, K, seed=2, scale=0.5), dtype)
    bias = rnd(N, seed=3)
    res = q(rnd(M, N, seed=4), dtype)
    pre_src = q(rnd(M, N, seed=5), dtype)
    tol = TOL[dtype] * (2 if dtype == torch.bfloat16 else 1)
    out = ops.gemm_nt(dev(A, dtype), dev(B, dtype))
    close(out, A @ B.t(), tol, "plain")
    pre = torch.empty(M, N, dtype=dtype, device="cuda")
    out = ops.gemm_nt(dev(A, dtype), dev(B, dtype), bias=dev(bias), act=1, preact=pre, residual=dev(res, dtype))
    ref_pre = A @ B.t() + bias
    close(pre, ref_pre, tol, "preact")
    close(out, O._gelu(ref_pre) + res, tol, "bias+gelu+residual")
    out = ops.gemm_nt(dev(A, dtype), dev(B, dtype), gelu_grad_of=dev(pre_src, dtype))
    x = pre_src.clone().requires_grad_(True)
    O._gelu(x).sum().backward()
    close(out, (A @ B.t()) * x.grad, tol, "gelu_grad epilogue")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_nt_dropout_is_a_scaled_mask_and_reproducible(ops, dtype):
    from sparse_hip import lib
    M, N, K = 256, 192, 64
    A, B = q(rnd(M, K, seed=1), dtype), q(rnd(N, K, seed=2), dtype)
    full = ops.gemm_nt(dev(A, dtype), dev(B, dtype)).float()
    d1 = ops.gemm_nt(dev(A, dtype), dev(B, dtype), drop=lib.dropout(0.1, 77, 3)).float()
    d2 = ops.gemm_nt(dev(A, dtype), dev(B, dtype), drop=lib.dropout(0.1, 77, 3)).float()
    d3 = ops.gemm_nt(dev(A, dtype), dev(B, dtype), drop=lib.dropout(0.1, 78, 3)).float()
    assert torch.equal(d1, d2)
    keep = d1 != 0
    frac = keep.float().mean().item()
    assert abs(frac - 0.9) < 0.01, frac
    assert (d3 != 0).ne(keep).any()
    p_q = int(0.1 * 256 + 0.5) / 256  # the rate actually applied: p rounded to 1/256 (include/sparse_hip.h, sm_dropout)
    close(d1[keep], (full / (1 - p_q))[keep], 2e-2 if dtype == torch.bfloat16 else 1e-3, "kept values are scaled by 1/(1-p_q)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_nt_dropout_mask_is_the_one_the_backward_kernels_regenerate(ops, dtype):
    """large (persistent-kernel) and small shapes must drop exactly the elements dropout_bwd drops for the same seed/site"""
    from sparse_hip import lib
    for M, N, K in ((8200, 384, 64), (96, 384, 64)):
        A, B = q(rnd(M, K, seed=1), dtype), q(rnd(N, K, seed=2), dtype)
        drop = lib.dropout(0.1, 123, 7)
        d1 = ops.gemm_nt(dev(A, dtype), dev(B, dtype), drop=drop).float()
        mask = ops.dropout_bwd(torch.ones(M, N, dtype=dtype, device="cuda"), drop).float()
        full = ops.gemm_nt(dev(A, dtype), dev(B, dtype)).float()
        assert torch.equal(d1 != 0, (mask != 0) & (full != 0))
        assert abs((mask != 0).float().mean().item() - 0.9) < 0.01


def test_gemm_nt_fused_with_layernorm_backward_matches_the_two_separate_kernels(ops):
    """input-gradient GEMM + residual + LayerNorm backward in one launch (N = hidden = 384, K >= 1024) against
    gemm_nt followed by layernorm_bwd, and against torch autograd in fp32"""
    from sparse_hip import lib
    dtype = torch.bfloat16
    # (6 k rows: one round of [128 x 384] tiles; 43 904 rows, the ragged bench batch: one round of [192 x 384] tiles; 65 536: two of 128)
    for M, K in ((6200, 1024), (6151, 1536), (6160, 384), (43904, 1536), (65536, 1152)):
        N = 384
        A, B = q(rnd(M, K, seed=1, scale=0.5), dtype), q(rnd(N, K, seed=2, scale=0.05), dtype)
        res, x = q(rnd(M, N, seed=3), dtype), q(rnd(M, N, seed=4, scale=2.0), dtype)
        gamma = 1.0 + 0.1 * rnd(N, seed=5)
        beta = 0.1 * rnd(N, seed=6)
        _, mean, rstd = ops.layernorm_fwd(dev(x, dtype), dev(gamma), dev(beta), 1e-12)
        drop = lib.dropout(0.1, 11, 5)
        dg0, db0 = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        dy = ops.gemm_nt(dev(A, dtype), dev(B, dtype), residual=dev(res, dtype))
        dx0, dxd0 = ops.layernorm_bwd(dy, dev(x, dtype), dev(gamma), mean, rstd, dg0, db0, drop, want_drop=True)
        dg1, db1 = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        out = ops.gemm_nt_ln_bwd(dev(A, dtype), dev(B, dtype), dev(res, dtype), dev(x, dtype), dev(gamma), mean, rstd, dg1, db1,
                                 drop, want_drop=True)
        assert out is not None, "the fused kernel must take this shape"
        dx1, dxd1 = out
        fro = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
        assert fro(dx1, dx0) <= 1e-2 and fro(dxd1, dxd0) <= 1e-2, (fro(dx1, dx0), fro(dxd1, dxd0))
        assert torch.equal(dxd1 != 0, (dx1 != 0) & (dxd0 != 0) | ((dxd1 != 0) & (dx0 == 0)))  # same dropout mask
        assert fro(dg1, dg0) <= 1e-2 and fro(db1, db0) <= 1e-2
        # fp32 autograd reference of LN' applied to the exact dy
        dyr = (A @ B.t() + res)
        xr = x.clone().requires_grad_(True)
        torch.nn.functional.layer_norm(xr, (N,), gamma, beta, 1e-12).backward(dyr)
        assert fro(dx1.cpu(), xr.grad) <= 2e-2
        # no residual (the head transform's input gradient), and the embedding form: dropout between the LayerNorm and dy
        dyd = lib.dropout(0.1, 77, 3)
        dy = ops.gemm_nt(dev(A, dtype), dev(B, dtype))
        dg0, db0 = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        dx0, _ = ops.layernorm_bwd(ops.dropout_bwd(dy, dyd), dev(x, dtype), dev(gamma), mean, rstd, dg0, db0)
        dg1, db1 = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        out = ops.gemm_nt_ln_bwd(dev(A, dtype), dev(B, dtype), None, dev(x, dtype), dev(gamma), mean, rstd, dg1, db1, dy_drop=dyd)
        assert out is not None and out[1] is None
        assert fro(out[0], dx0) <= 1e-2 and fro(dg1, dg0) <= 1e-2 and fro(db1, db0) <= 1e-2, (fro(out[0], dx0), fro(dg1, dg0))
    # shapes the fused kernel does not take are declined, not mis-computed
    A, B = dev(q(rnd(500, 1024, seed=1), dtype), dtype), dev(q(rnd(384, 1024, seed=2), dtype), dtype)
    xs = dev(q(rnd(500, 384, seed=3), dtype), dtype)
    _, mean, rstd = ops.layernorm_fwd(xs, dev(torch.ones(384)), dev(torch.zeros(384)), 1e-12)
    z = torch.zeros(384, device="cuda")
    assert ops.gemm_nt_ln_bwd(A, B, xs, xs, dev(torch.ones(384)), mean, rstd, z, z.clone()) is None


def test_gemm_nt_residual_recomputed_from_the_layernorm_input(ops):
    """fp32 residual stream without storing the fp32 LayerNorm outputs: residual_ln = (mean, rstd, gamma, beta) makes the
    epilogue add LayerNorm(residual) -- against the same GEMM fed the stored fp32 LayerNorm output (both GEMM kernels)"""
    from sparse_hip import lib
    dtype = torch.bfloat16
    N = 384
    for M, K in ((6200, 384), (6200, 1536), (333, 384)):
        A, B = dev(q(rnd(M, K, seed=1, scale=0.5), dtype), dtype), dev(q(rnd(N, K, seed=2, scale=0.05), dtype), dtype)
        z = dev(rnd(M, N, seed=3, scale=1.5) + 0.2)
        gamma, beta, bias = dev(1.0 + 0.1 * rnd(N, seed=4)), dev(0.1 * rnd(N, seed=5)), dev(0.1 * rnd(N, seed=6))
        y, y32, mean, rstd = ops.layernorm_fwd_res32(z, gamma, beta, 1e-12, dtype)
        assert ops.layernorm_fwd_res32(z, gamma, beta, 1e-12, dtype, want_y32=False)[1] is None
        drop = lib.dropout(0.1, 5, 2)
        want = ops.gemm_nt(A, B, bias=bias, drop=drop, residual=y32, out_f32=True)
        got = ops.gemm_nt(A, B, bias=bias, drop=drop, residual=z, out_f32=True, residual_ln=(mean, rstd, gamma, beta))
        assert got.dtype == torch.float32 and float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), (M, K)


@pytest.mark.parametrize("M", [8192, 8300, 43904])
@pytest.mark.parametrize("with_ln", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gemm_nt_fp32_residual_epilogue_of_the_weight_stationary_kernel(ops, M, with_ln, p):
    """the attention-output projection of the fp32 residual stream at K = 384 and >= 8192 rows runs in the weight-stationary kernel
    (gemm_ws.hip, EPI 2): fp32 out = dropout(A.W^T + bias) + residual, the residual being the fp32 tensor itself or LayerNorm of it
    recomputed from (mean, rstd, gamma, beta).  Against fp32 torch on the same bf16 operands with the dropout mask the backward
    kernels regenerate (sm_dropout_bwd on ones); a row count that ends inside a 32-row step"""
    from sparse_hip import lib
    dtype = torch.bfloat16
    N = K = 384
    A, B = q(rnd(M, K, seed=1, scale=0.5), dtype), q(rnd(N, K, seed=2, scale=0.05), dtype)
    z = rnd(M, N, seed=3, scale=1.5) + 0.2
    gamma, beta, bias = 1.0 + 0.1 * rnd(N, seed=4), 0.1 * rnd(N, seed=5), 0.1 * rnd(N, seed=6)
    zd = dev(z)
    drop = lib.dropout(p, 5, 2) if p else None
    ln = None
    res = z
    if with_ln:
        _, _, mean, rstd = ops.layernorm_fwd_res32(zd, dev(gamma), dev(beta), 1e-12, dtype)
        ln = (mean, rstd, dev(gamma), dev(beta))
        res = torch.nn.functional.layer_norm(z, (N,), gamma, beta, 1e-12)
    got = ops.gemm_nt(dev(A, dtype), dev(B, dtype), bias=dev(bias), drop=drop, residual=zd, out_f32=True, residual_ln=ln)
    lin = A @ B.t() + bias
    if p:
        keep = ops.dropout_bwd(torch.ones(M, N, dtype=dtype, device="cuda"), drop).float().cpu() != 0
        p_q = int(p * 256 + 0.5) / 256  # the rate actually applied (include/sparse_hip.h, sm_dropout)
        lin = lin * keep / (1 - p_q)
    want = lin + res
    assert got.dtype == torch.float32
    close(got, want, 2e-5 if not with_ln else 1e-4, "fp32 residual epilogue")


@pytest.mark.parametrize("density", [0.0, 0.002, 0.05])
@pytest.mark.parametrize("ragged", [False, True])
def test_head_dt_with_few_live_activations_skips_steps_without_changing_the_sum(ops, density, ragged):
    """dt = G . E (head_dt192_kernel) skips the MFMAs of a 32-column step whose G slice is all zero for the tile's documents -- the
    common step once the model is sparse.  Against a float64 evaluation of the routed sum: a few live columns, whole documents
    without any, runs of live columns next to runs of dead ones, nothing alive at all; dense and ragged rows"""
    dtype = torch.bfloat16
    H, V = 384, 4000
    g = torch.Generator().manual_seed(int(density * 1e4) + ragged)
    if ragged:
        lens = [37, 128, 16, 90, 5, 64, 128, 77]
        _, off_np, rows, row_doc, pos, _ = _ragged(lens)
        B, S = len(lens), 128
        rag = ops.Ragged(dev(off_np.astype(np.int32)), dev(row_doc[::16].astype(np.int32)), dev(pos.astype(np.int32)), rows, B, S)
        off = off_np.tolist()
    else:
        B, S, rag = 7, 128, None
        lens, off, rows = [S] * B, [i * S for i in range(B + 1)], B * S
    E = torch.randn(V, H, generator=g).mul(0.2).to(dtype)
    rep = (torch.rand(B, V, generator=g) + 0.05) * (torch.rand(B, V, generator=g) < density)
    rep[1, 640:704] = 0.3            # a run of live columns in one document
    rep[2] = 0.0                     # a document without any
    if density == 0.0:
        rep.zero_()
    grad = torch.randn(B, V, generator=g)
    am = torch.stack([torch.randint(0, lens[b], (V,), generator=g) for b in range(B)]).to(torch.int16)
    dt = ops.sparse_head_bwd(dev(grad), dev(rep), dev(am).view(torch.uint16), torch.empty(rows, H, device="cuda", dtype=dtype), dev(E, dtype), None, None,
                             B, S, V, False, rag, part="dt")
    gr = grad.double() * torch.where(rep > 0, torch.exp(-rep.double()), torch.zeros(B, V, dtype=torch.float64))
    want = torch.zeros(rows, H, dtype=torch.float64)
    for b in range(B):
        want.index_add_(0, off[b] + am[b].long(), gr[b][:, None] * E.double())
    scale = max(float(want.abs().max()), 1e-6)
    # (the kernel rounds G to bf16 and its result to bf16)
    assert float((dt.float().cpu().double()[:rows] - want).abs().max()) <= 1.2e-2 * scale, density
    if density == 0.0:
        assert float(dt.float().abs().max()) == 0.0


@pytest.mark.parametrize("live", [1.0, 0.01])
def test_head_backward_fused_with_the_transform_layernorm_and_gelu_backward(ops, live):
    """dt = G.E never goes to HBM: LayerNorm' and GELU' of the head transform run in the kernel's epilogue (bf16, H = 384);
    against sparse_head_bwd(dt) -> layernorm_bwd -> gelu_bwd.  live = 0.01: gradient on 1 % of the entries only (most 32-column steps
    are skipped by both forms)"""
    dtype = torch.bfloat16
    B, S, H, V = 24, 128, 384, 3000
    t = q(rnd(B * S, H, seed=1), dtype)
    E = q(rnd(V, H, seed=2, scale=0.2), dtype)
    bias = 0.1 * rnd(V, seed=3)
    mask = (torch.arange(S)[None, :] < torch.randint(20, S + 1, (B, 1), generator=torch.Generator().manual_seed(4))).to(torch.uint8)
    rep, argmax = ops.sparse_head_fwd(dev(t, dtype), dev(E, dtype), dev(bias), dev(mask, torch.uint8), B, S, V, False, None)
    grad_rep = dev(rnd(B, V, seed=5).abs() * (torch.rand(B, V, generator=torch.Generator().manual_seed(11)) < live))
    gt = q(rnd(B * S, H, seed=6, scale=1.5), dtype)   # LayerNorm input
    ft = q(rnd(B * S, H, seed=7), dtype)              # GELU input
    gamma, beta = 1.0 + 0.1 * rnd(H, seed=8), 0.1 * rnd(H, seed=9)
    _, mean, rstd = ops.layernorm_fwd(dev(gt, dtype), dev(gamma), dev(beta), 1e-12)
    dE, db = torch.zeros(V, H, device="cuda"), torch.zeros(V, device="cuda")
    dt = ops.sparse_head_bwd(grad_rep, rep, argmax, dev(t, dtype), dev(E, dtype), dE, db, B, S, V, False, None, part="dt")
    dg0, db0 = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
    dgt, _ = ops.layernorm_bwd(dt, dev(gt, dtype), dev(gamma), mean, rstd, dg0, db0)
    dft0 = ops.gelu_bwd(dgt, dev(ft, dtype))
    dg1, db1 = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
    dft1 = ops.sparse_head_bwd_dt_ln(grad_rep, rep, argmax, dev(E, dtype), B, S, V, False, None, dev(gt, dtype), dev(gamma), mean, rstd,
                                     dev(ft, dtype), dg1, db1)
    assert dft1 is not None, "the fused kernel must take this shape"
    fro = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    assert fro(dft1, dft0) <= 1e-2 and fro(dg1, dg0) <= 1e-2 and fro(db1, db0) <= 1e-2, (fro(dft1, dft0), fro(dg1, dg0), fro(db1, db0))
    assert float((dft1.float() - dft0.float()).abs().max()) <= 2e-2 * float(dft0.float().abs().max())
    # other hidden sizes are declined
    x256 = dev(q(rnd(B * S, 256, seed=1), dtype), dtype)
    assert ops.sparse_head_bwd_dt_ln(grad_rep, rep, argmax, dev(q(rnd(V, 256, seed=2), dtype), dtype), B, S, V, False, None, x256, dev(torch.ones(256)),
                                     mean, rstd, x256, torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda")) is None


@pytest.mark.parametrize("B,S,V,ragged", [(60, 128, 8192, False), (60, 128, 8192, True), (512, 128, 30522, False), (300, 128, 30522, False)])
def test_head_backward_split_tail_equals_the_whole_tile_form(ops, B, S, V, ragged):
    """sm_sparse_head_bwd_dt_ln with its workspace (ABI 6): a last round of 192-row tiles that would leave most of the chip idle is split
    along the vocabulary, partial tiles summed with fp32 atomics, a small third launch runs the LayerNorm' / GELU' epilogue on the sums.  Same
    result as the whole-tile form up to fp32 summation order; the workspace is zero again afterwards (the next launch relies on it).
    40 tiles (all split, runs straddle tiles), the bench batch (342 = 256 whole + 86 split), 200 tiles (> 3/4 of the chip: not split)"""
    dtype = torch.bfloat16
    H = 384
    g = torch.Generator().manual_seed(B + V)
    if ragged:
        lens = (torch.randint(4, S // 16 + 1, (B,), generator=g) * 16 - 3).tolist()
        lens[0] = S
        _, off_np, nrows, row_doc, pos, _ = _ragged(lens)
        rag = ops.Ragged(dev(off_np.astype(np.int32)), dev(row_doc[::16].astype(np.int32)), dev(pos.astype(np.int32)), nrows, B, S)
    else:
        lens, rag, nrows = [S] * B, None, B * S
    E = dev(q(rnd(V, H, seed=2, scale=0.2), dtype), dtype)
    rep = dev(torch.rand(B, V, generator=g) * (torch.rand(B, V, generator=g) < 0.3))
    grad_rep = dev(torch.randn(B, V, generator=g))
    argmax = dev(torch.stack([torch.randint(0, lens[b], (V,), generator=g) for b in range(B)]).to(torch.int16)).view(torch.uint16)
    gt, ft = dev(q(rnd(nrows, H, seed=6, scale=1.5), dtype), dtype), dev(q(rnd(nrows, H, seed=7), dtype), dtype)
    gamma, beta = dev(1.0 + 0.1 * rnd(H, seed=8)), dev(0.1 * rnd(H, seed=9))
    _, mean, rstd = ops.layernorm_fwd(gt, gamma, beta, 1e-12)
    out = []
    for split in (False, True, True):
        dg, db = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
        dft = ops.sparse_head_bwd_dt_ln(grad_rep, rep, argmax, E, B, S, V, False, rag, gt, gamma, mean, rstd, ft, dg, db, split_tail=split)
        assert dft is not None
        out.append((dft.float().cpu(), dg.cpu(), db.cpu()))
    (ws,) = [w for (d_, _), w in ops._DT_WS.items() if d_ == torch.cuda.current_device()]  # one per (device, stream); this process used one stream
    assert float(ws.abs().max()) == 0.0, "the split tail must leave its workspace zero"
    scale = float(out[0][0].abs().max())
    for k in (1, 2):  # (twice: the second launch starts from the workspace the first one left)
        assert float((out[k][0] - out[0][0]).abs().max()) <= 4e-3 * scale  # one bf16 ulp of the largest entry
        assert float((out[k][0] - out[0][0]).norm() / out[0][0].norm()) <= 1e-3
        for a in (1, 2):
            assert float((out[k][a] - out[0][a]).norm() / out[0][a].norm()) <= 1e-3


# ------------------------------------------------------------------ GEMM TN
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,Kc", [(300, 72, 136), (1024, 128, 128), (96, 192, 64), (2000, 64, 520 - 520 % 8),
                                    (4096, 384, 256), (2080, 128, 384), (2064, 128, 384), (43, 128, 128), (1000, 256, 128),
                                    (8200, 384, 384), (33, 128, 256)])
def test_gemm_tn_acc(ops, dtype, M, N, Kc):
    A, B = q(rnd(M, N, seed=1, scale=0.5), dtype), q(rnd(M, Kc, seed=2, scale=0.5), dtype)
    init = rnd(N, Kc, seed=3)
    out = dev(init.clone())
    cs = torch.zeros(N, device="cuda")
    ops.gemm_tn_acc(dev(A, dtype), dev(B, dtype), out, colsum=cs)
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    close(out, init + A.t() @ B, tol, "A^T B accumulate")
    close(cs, A.sum(0), tol, "column sums")


def _to_bcm(x: torch.Tensor) -> torch.Tensor:
    """row-major [rows, cols] -> the block-column-major buffer of sm_ffn_pc_bwd's outputs: [ceil(rows / 128) * 4][cols / 8][32][8]"""
    rows, cols = x.shape
    rp = (rows + 127) // 128 * 128
    pad = torch.zeros(rp, cols, dtype=x.dtype)
    pad[:rows] = x
    return pad.reshape(rp // 32, 32, cols // 8, 8).permute(0, 2, 1, 3).contiguous()


@pytest.mark.parametrize("M,layers", [(32, 1), (100, 1), (1000, 1), (4112, 1), (70000, 1), (300, 2), (43904, 2)])
def test_gemm_tn_group_matches_fp32_products(ops, M, layers):
    """the grouped weight-gradient kernel (csrc/gemm_tn2.hip, hf:175-177 / :290 / :335 / :348 backward in ONE launch): every product
    against the fp32 product of the same bf16 operands, accumulating into a non-zero C; row counts that are not multiples of the
    32-row stage, one stage only, and more rows than one split; operands with a leading dimension, block-column-major operands,
    problems with and without a bias gradient; the products of ONE layer, and of two (the inner layers of the backward go in pairs)"""
    dt = torch.bfloat16
    shapes = [(1152, 384), (384, 384), (1536, 384), (384, 1536)] * layers
    probs, want = [], []
    for n, (N, Kc) in enumerate(shapes):
        i = n % 4
        A, B = q(rnd(M, N, seed=10 + n, scale=0.5), dt), q(rnd(M, Kc, seed=20 + n, scale=0.5), dt)
        init = rnd(N, Kc, seed=30 + n)
        out = dev(init.clone())
        cs = torch.full((N,), 0.5, device="cuda") if n != 1 else None
        a_dev, b_dev = dev(A, dt), dev(B, dt)
        if i == 2:  # FFN up: dF1 block-column-major (A), x1 row-major
            a_dev = ops.Bcm(dev(_to_bcm(A.to(dt))), M, N)
        if i == 3:  # FFN down: gelu(f1) block-column-major (B)
            b_dev = ops.Bcm(dev(_to_bcm(B.to(dt))), M, Kc)
        if i == 0:  # a view with a leading dimension (the fused QKV gradient is one: lda > N)
            wide = torch.zeros(M, N + 64, dtype=dt, device="cuda")
            wide[:, :N] = a_dev
            a_dev = wide[:, :N]
        probs.append((a_dev, b_dev, out, cs))
        want.append((init + A.t() @ B, None if cs is None else 0.5 + A.sum(0)))
    assert ops.gemm_tn_group(probs), "the grouped kernel declined the encoder's own shapes"
    for (a, b, out, cs), (w, wcs), (N, Kc) in zip(probs, want, shapes):
        close(out, w, 1e-2, f"A^T B accumulate [{N} x {Kc}]")
        rel = float((out.cpu() - w).norm() / w.norm())
        assert rel <= 2e-5 + 1e-6 * math.sqrt(M), f"[{N} x {Kc}]: relative Frobenius error {rel:.2e} (fp32 accumulation of exact bf16 products)"
        if cs is not None:
            close(cs, wcs, 1e-2, f"column sums [{N}]")


def test_gemm_tn_group_equals_the_per_matrix_kernel_and_declines_other_shapes(ops):
    dt = torch.bfloat16
    M = 5000
    A, B = dev(q(rnd(M, 768, seed=1, scale=0.5), dt), dt), dev(q(rnd(M, 2304, seed=2, scale=0.5), dt), dt)
    o1, o2 = torch.zeros(768, 2304, device="cuda"), torch.zeros(768, 2304, device="cuda")
    c1, c2 = torch.zeros(768, device="cuda"), torch.zeros(768, device="cuda")
    assert ops.gemm_tn_group([(A, B, o1, c1)])  # bert-base width: 4 x 12 tiles
    ops.gemm_tn_acc(A, B, o2, colsum=c2)
    close(o1, o2, 1e-5, "grouped vs per-matrix kernel")  # both accumulate exact products in fp32: only the summation order differs
    close(c1, c2, 1e-5, "column sums")
    # N a multiple of 192 but not of 384: the [192 x 192] loader / consumer kernel instead of the symmetric [384 x 192] one
    A5, B5 = dev(q(rnd(M, 576, seed=3, scale=0.5), dt), dt), dev(q(rnd(M, 192, seed=4, scale=0.5), dt), dt)
    o5, c5 = torch.zeros(576, 192, device="cuda"), torch.zeros(576, device="cuda")
    assert ops.gemm_tn_group([(A5, B5, o5, c5)])
    close(o5, A5.float().t() @ B5.float(), 1e-5, "[576 x 192] through the [192 x 192] kernel")
    close(c5, A5.float().sum(0), 1e-5, "its column sums")
    # not a multiple of 192 / fp32 operands / nine problems: declined, nothing launched
    o3 = torch.zeros(128, 384, device="cuda")
    assert not ops.gemm_tn_group([(A[:, :128].contiguous(), B[:, :384].contiguous(), o3, None)])
    assert float(o3.abs().max()) == 0.0
    assert not ops.gemm_tn_group([(A.float(), B.float(), o1, None)])
    assert not ops.gemm_tn_group([(A, B, o1, None)] * 9)


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,H", [(37, 64), (130, 384), (9, 768), (301, 768), (77, 1024)])
def test_layernorm_fwd_bwd(ops, dtype, rows, H):
    x = q(rnd(rows, H, seed=1) * 2 + 0.3, dtype)
    gamma, beta = 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)
    dy = q(rnd(rows, H, seed=4), dtype)
    y, mean, rstd = ops.layernorm_fwd(dev(x, dtype), dev(gamma), dev(beta), 1e-12)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = O._ln(xr, gr, br, 1e-12)
    tol = TOL[dtype]
    close(y, yr, tol * 2, "y")
    close(mean, x.mean(-1), 1e-4, "mean")
    (yr * dy).sum().backward()
    dg, db = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
    dx, _ = ops.layernorm_bwd(dev(dy, dtype), dev(x, dtype), dev(gamma), mean, rstd, dg, db)
    close(dx, xr.grad, tol * 2, "dx")
    close(dg, gr.grad, tol * 2, "dgamma")
    close(db, br.grad, tol * 2, "dbeta")


# ------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_fwd_bwd(ops, dtype):
    B, S, H, V = 5, 16, 64, 300
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, V, (B, S), generator=g)
    word = q(rnd(V, H, seed=1, scale=0.1), dtype)
    pos, typ = rnd(32, H, seed=2, scale=0.1), rnd(H, seed=3, scale=0.1)
    gamma, beta = 1 + 0.1 * rnd(H, seed=4), 0.1 * rnd(H, seed=5)
    z, y, mean, rstd = ops.embed_fwd(dev(ids), dev(word, dtype), dev(pos), dev(typ), dev(gamma), dev(beta), 1e-12)
    zr = word[ids] + pos[:S] + typ
    close(z.view(B, S, H), zr, TOL[dtype], "z")
    close(y.view(B, S, H), O._ln(q(zr, dtype), gamma, beta, 1e-12), TOL[dtype] * 3, "y")
    dz = q(rnd(B * S, H, seed=6), dtype)
    gw, gp, gt = torch.zeros(V, H, device="cuda"), torch.zeros(32, H, device="cuda"), torch.zeros(H, device="cuda")
    ops.embed_bwd(dev(dz, dtype), dev(ids), gw, gp, gt)
    rw = torch.zeros(V, H).index_add_(0, ids.reshape(-1), dz)
    close(gw, rw, 1e-4, "word grad")
    close(gp[:S], dz.view(B, S, H).sum(0), 1e-4, "pos grad")
    close(gt, dz.sum(0), 1e-4, "type grad")


@pytest.mark.parametrize("H,V", [(128, 500), (384, 500), (768, 500), (384, 30522), (256, 3000)])
def test_embed_bwd_from_host_sorted_rows_matches_the_scatter(ops, H, V):
    """packed layout, bf16: run sums over the rows sorted by token id / by position (pack_documents -> rag.emb_sorted; [CLS] /
    [SEP] in every document, a token repeated 100 times) against index_add in fp32 and against the atomic scatter kernel.
    V = 30522 / 3000 (round 6): most token ids occur once or twice (runs of one entry, the bench's synthetic ids), while [CLS] / [SEP] /
    the repeated token span waves; the tables already hold values (the tied head gradient is added first)"""
    from sparse_hip.encoder import pack_documents
    dtype = torch.bfloat16
    B, S = 150, 64
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    ids = torch.randint(10, V, (B, S), generator=g)
    ids[:, 0] = 101
    ids[torch.arange(B), lens - 1] = 102
    ids[:100, 1] = 7
    mask = (torch.arange(S)[None, :] < lens[:, None]).long()
    ids = ids * mask
    pk = pack_documents(ids, mask, "cuda")
    assert pk is not None and pk.rag.emb_sorted is not None
    rows = pk.rag.rows
    dz = q(rnd(rows, H, seed=6), dtype) * pk.mask.cpu()[:, None].float()  # padding rows carry a zero gradient
    out = {}
    for name in ("sorted", "scatter"):
        base = [dev(rnd(V, H, seed=11)), dev(rnd(S, H, seed=12)), dev(rnd(H, seed=13))]  # accumulate semantics: the tables are not zero
        gw, gp, gt = (t.clone() for t in base)
        srt = pk.rag.emb_sorted
        if name == "scatter":
            pk.rag.emb_sorted = None
        ops.embed_bwd(dev(dz, dtype), pk.ids, gw, gp, gt, pk.rag)
        pk.rag.emb_sorted = srt
        out[name] = ((gw - base[0]).cpu(), (gp - base[1]).cpu(), (gt - base[2]).cpu())
    pid, ppos = pk.ids.cpu(), pk.rag.pos_ids.cpu().long()
    rw = torch.zeros(V, H).index_add_(0, pid, dz)
    rp = torch.zeros(S, H).index_add_(0, ppos, dz)
    for name, (gw, gp, gt) in out.items():
        close(gw, rw, 1e-4, name + " word grad")
        close(gp, rp, 1e-4, name + " pos grad")
        close(gt, dz.sum(0), 1e-4, name + " type grad")


def test_loss_combine_scalar_tail(ops):
    """ranking = sum w_i l_i; total = ranking + lambda_d flops_d + lambda_q flops_q; moving average updated in place (trainer.py:101-141)"""
    l = [torch.tensor([v], device="cuda") for v in (1.25, 0.5, 3.0)]
    fd, fq = torch.tensor([2.0], device="cuda"), torch.tensor([0.75], device="cuda")
    ma = torch.tensor([10.0], device="cuda")
    ranking, total = ops.loss_combine([(l[0], 1.0), (l[1], 0.5), (l[2], 2.0)], fd, 0.1, fq, 0.01, ma, 0.01)
    assert abs(float(ranking) - 7.5) < 1e-6 and abs(float(total) - (7.5 + 0.2 + 0.0075)) < 1e-6
    assert abs(float(ma) - (0.01 * 7.5 + 0.99 * 10.0)) < 1e-5
    ranking, total = ops.loss_combine([(l[0], 1.0)], fd, 0.5, None, 0.0)
    assert abs(float(ranking) - 1.25) < 1e-6 and abs(float(total) - 2.25) < 1e-6
    with pytest.raises(Exception, match="at most 4"):
        ops.loss_combine([(l[0], 1.0)] * 5, fd, 0.5, None, 0.0)


# ------------------------------------------------------------------ attention
def ref_attention(qkv, mask, B, S, A, dh):
    H = A * dh
    x = qkv.view(B, S, 3, A, dh)
    qq, kk, vv = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    s = qq @ kk.transpose(-1, -2) / math.sqrt(dh)
    s = s + (1.0 - mask.float())[:, None, None, :] * torch.finfo(torch.float32).min
    p = torch.softmax(s, -1)
    return (p @ vv).transpose(1, 2).reshape(B * S, H), torch.logsumexp(s, -1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,A,dh", [(3, 32, 2, 32), (2, 64, 3, 32), (2, 128, 2, 64), (2, 128, 12, 32), (1, 256, 2, 32), (2, 256, 3, 64),
                                     (2, 512, 2, 32), (2, 512, 2, 64)])
def test_attention_fwd_bwd(ops, dtype, B, S, A, dh):
    if dtype == torch.float32 and S * dh > 256 * 64:
        pytest.skip("fp32 parity mode: two [S][dh] fp32 LDS images cap S*dh at 256*64")
    H = A * dh
    qkv = q(rnd(B * S, 3 * H, seed=1), dtype)
    mask = torch.ones(B, S, dtype=torch.uint8)
    for b in range(1, B):
        mask[b, S - 5 * b - 3:] = 0
    dctx = q(rnd(B * S, H, seed=2), dtype)
    ctx, lse = ops.attention_fwd(dev(qkv, dtype), dev(mask), B, S, A)
    xr = qkv.clone().requires_grad_(True)
    cr, lr = ref_attention(xr, mask, B, S, A, dh)
    tol = TOL[dtype] * 2
    close(ctx, cr, tol, "ctx")
    close(lse, lr, 2e-3 if dtype == torch.float32 else 2e-2, "lse")
    (cr * dctx).sum().backward()
    dqkv = ops.attention_bwd(dev(qkv, dtype), dev(mask), ctx, dev(dctx, dtype), lse, B, S, A)
    close(dqkv, xr.grad, tol * 2, "dqkv")


@pytest.mark.parametrize("S", [128, 256, 512])
def test_attention_dense_layout_skips_only_the_masked_tail(ops, S):
    """dense [B, S] batches: key tiles behind the LAST attended key are not computed (their probabilities are exactly zero).  Masks that
    are not prefixes (holes, a single attended key at the end, nothing attended at all, lengths on and off the 16 / 32 boundaries)
    must give the same context rows and gradients as the full computation.  S = 256 / 512 (round 6): the 8-wave forward and the
    single-pass backward attn_bwd2_kernel, whose key-block loop ends at the last attended key"""
    B, A, dh = 8, 2, 32
    H = A * dh
    f = S // 128
    dtype = torch.bfloat16
    qkv = q(rnd(B * S, 3 * H, seed=1), dtype)
    mask = torch.zeros(B, S, dtype=torch.uint8)
    mask[0, :] = 1
    mask[1, :16] = 1
    mask[2, :33 * f] = 1
    mask[3, :96 * f] = 1
    mask[3, 20 * f:70 * f] = 0    # a hole
    mask[4, S - 1] = 1            # only the last key
    mask[5, :1] = 1               # only the first key
    mask[6, :64 * f + (3 if f > 1 else 0)] = 1
    # document 7: nothing attended
    dctx = q(rnd(B * S, H, seed=2), dtype) * mask.view(-1, 1)
    ctx, lse = ops.attention_fwd(dev(qkv, dtype), dev(mask), B, S, A)
    dqkv = ops.attention_bwd(dev(qkv, dtype), dev(mask), ctx, dev(dctx, dtype), lse, B, S, A)
    live = [b for b in range(B) if int(mask[b].sum()) > 0]
    xr = qkv.clone().requires_grad_(True)
    sel = torch.cat([torch.arange(b * S, (b + 1) * S) for b in live])
    cr, _ = ref_attention(xr[sel], mask[live], len(live), S, A, dh)
    tol = TOL[dtype] * 2
    close(ctx.float().cpu()[sel], cr, tol, "ctx")
    (cr * dctx[sel]).sum().backward()
    close(dqkv.float().cpu()[sel], xr.grad[sel], tol * 2, "dqkv")
    assert float(ctx.float().cpu()[7 * S:].abs().max()) == 0.0 and float(dqkv.float().cpu()[7 * S:].abs().max()) == 0.0
    assert bool(torch.isfinite(dqkv.float()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_dropout_consistent_between_fwd_and_bwd(ops, dtype):
    """finite-difference-free check: with dropout the backward must be the exact gradient of
    the forward for the same mask -> compare a directional derivative."""
    from sparse_hip import lib
    B, S, A, dh = 2, 64, 2, 32
    H = A * dh
    drop = lib.dropout(0.1, 5, 9)
    base = rnd(B * S, 3 * H, seed=1) * 0.5
    direction = rnd(B * S, 3 * H, seed=2)
    mask = torch.ones(B, S, dtype=torch.uint8)
    dctx = rnd(B * S, H, seed=3)
    if dtype == torch.bfloat16:
        pytest.skip("directional derivative needs fp32 resolution")
    eps = 1e-2
    f = lambda x: (ops.attention_fwd(dev(x), dev(mask), B, S, A, drop)[0].cpu() * dctx).sum().item()
    ctx, lse = ops.attention_fwd(dev(base), dev(mask), B, S, A, drop)
    dqkv = ops.attention_bwd(dev(base), dev(mask), ctx, dev(dctx), lse, B, S, A, drop).cpu()
    num = (f(base + eps * direction) - f(base - eps * direction)) / (2 * eps)
    ana = (dqkv * direction).sum().item()
    assert abs(num - ana) <= 2e-2 * max(1.0, abs(ana)), (num, ana)
    ctx0, _ = ops.attention_fwd(dev(base), dev(mask), B, S, A)
    assert not torch.equal(ctx0, ctx)


# ------------------------------------------------------------------ fused sparse head
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,V", [(6, 16, 64, 520), (5, 64, 128, 300), (3, 128, 128, 1000), (2, 256, 128, 260), (2, 512, 128, 260),
                                     (2, 256, 384, 300), (3, 512, 384, 260), (3, 128, 384, 700), (5, 64, 384, 300), (5, 32, 384, 300)])
@pytest.mark.parametrize("use_l0", [False, True])
def test_sparse_head_fwd_bwd(ops, dtype, B, S, H, V, use_l0):
    t = q(rnd(B * S, H, seed=1), dtype)
    E = q(rnd(V, H, seed=2, scale=0.3), dtype)
    bias = rnd(V, seed=3, scale=0.5)
    mask = torch.ones(B, S, dtype=torch.uint8)
    for b in range(1, B):
        mask[b, S - 3 * b - 2:] = 0
    rep, am = ops.sparse_head_fwd(dev(t, dtype), dev(E, dtype), dev(bias), dev(mask), B, S, V, use_l0)
    tr, Er, br = t.clone().requires_grad_(True), E.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    logits = (tr @ Er.t() + br).view(B, S, V)
    ref = O.sparse_activation(logits, mask.long(), use_l0)
    tol = TOL[dtype] * 2
    close(rep, ref, tol, "rep")
    # argmax must point at an ATTENDED position that attains the max.  fp32: exactly (1e-4).  16-bit operands: the vocabulary-stationary
    # kernels carry the position in the low 7-9 mantissa bits of the maximum, so two positions whose values agree to 2^-14 relative
    # may swap (documented in csrc/head_fwd.hip) -- the bound asserted is four times that window, not round 5's 5e-2
    pos = am.cpu().long() & 0xFFFF
    masked = logits.detach().masked_fill(mask[:, :, None] == 0, -float("inf"))
    picked = torch.gather(masked, 1, pos[:, None, :]).squeeze(1)
    live = ref > 0
    top = masked.max(1).values
    assert (picked[live] >= top[live] - (1e-4 if dtype == torch.float32 else 2.0 ** -12 * (top[live].abs() + br.detach().abs().max() + 1))).all()
    up = rnd(B, V, seed=4)
    if dtype != torch.float32:  # the reference gradient flows to the position the device chose among such near-ties (checked above)
        ref = O.sparse_activation(logits, mask.long(), use_l0, route=pos)
    (ref * up).sum().backward()
    dE = torch.zeros(V, H, device="cuda")
    dbias = torch.zeros(V, device="cuda")
    dt = ops.sparse_head_bwd(dev(up), rep, am, dev(t, dtype), dev(E, dtype), dE, dbias, B, S, V, use_l0)
    close(dt, tr.grad, tol * 2, "dt")
    close(dE, Er.grad, tol * 2, "dE")
    close(dbias, br.grad, tol * 2, "dbias")


@pytest.mark.parametrize("H,B,S,V", [(384, 9, 128, 30522), (384, 3, 16, 130), (768, 11, 128, 2100), (128, 7, 32, 1025)])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("density", [0.01, 0.6])
def test_head_dt_scatter_is_the_routed_sum_in_fp32(ops, H, B, S, V, ragged, density):
    """dt half of the head backward as a scatter over the live entries (head_dt_scatter_kernel, the trained-checkpoint regime):
    dt[row(d) + argmax[d, v]] += g[d, v] E[v] in fp32, rounded to bf16 once -- against a float64 evaluation, at 1 % and 60 % of the
    activations alive, dense and ragged layouts, a vocabulary that is no multiple of the 1024 columns of a workgroup; and against
    the matrix form (head_dt192 / head_dt_mfma), which rounds G to bf16 first"""
    g = torch.Generator().manual_seed(H + B + int(density * 100))
    if ragged:
        lens = (torch.randint(1, S // 16 + 1, (B,), generator=g) * 16).tolist()
        _, off_np, rows, row_doc, pos, _ = _ragged(lens)
        rag = ops.Ragged(dev(off_np.astype(np.int32)), dev(row_doc[::16].astype(np.int32)), dev(pos.astype(np.int32)), rows, B, S)
        off = off_np.tolist()
    else:
        lens, off, rag = [S] * B, [i * S for i in range(B + 1)], None
    T = off[-1]
    E = (torch.randn(V, H, generator=g) * 0.3).to(torch.bfloat16)
    rep = torch.rand(B, V, generator=g) + 0.05
    rep[torch.rand(B, V, generator=g) >= density] = 0.0
    rep[B // 2] = 0.0                     # a document without any gradient
    grad = torch.randn(B, V, generator=g)
    am = torch.stack([torch.randint(0, lens[b], (V,), generator=g) for b in range(B)]).to(torch.int16)
    args = (dev(grad), dev(rep), dev(am).view(torch.uint16), dev(E, torch.bfloat16), B, S, V, False, rag)
    dt = ops.sparse_head_bwd_dt_scatter(*args, T)
    gr = grad.double() * torch.where(rep > 0, torch.exp(-rep.double()), torch.zeros(B, V, dtype=torch.float64))
    want = torch.zeros(T, H, dtype=torch.float64)
    for b in range(B):
        want.index_add_(0, off[b] + am[b].long(), gr[b][:, None] * E.double())
    scale = float(want.abs().max())
    err = float((dt.double().cpu() - want).abs().max())
    assert err <= 2 ** -8 * scale, f"scatter vs float64: {err:.3e} of {scale:.3e}"  # one bf16 rounding of the fp32 sum
    dtm = ops.sparse_head_bwd(args[0], args[1], args[2], torch.zeros(T, H, dtype=torch.bfloat16, device="cuda"), args[3], None, None, B, S, V,
                              False, rag, part="dt")
    assert float((dtm.double().cpu() - want).abs().max()) <= 2e-2 * scale  # the matrix form: G rounded to bf16 before the product
    assert float((dtm.float() - dt.float()).abs().max()) <= 2e-2 * scale


@pytest.mark.parametrize("H,B,S,V", [(128, 7, 32, 333), (256, 5, 64, 1000), (384, 9, 128, 30522), (384, 1, 16, 130), (512, 6, 48, 257),
                                     (768, 11, 128, 2100), (1024, 18, 16, 515)])
@pytest.mark.parametrize("ragged", [False, True])
def test_head_de_row_gathers_are_the_routed_sum_in_fp32(ops, H, B, S, V, ragged):
    """dE / dbias half of the head backward for bf16 rows (head_de_rows_kernel): dE[v] += sum_d g[d, v] t[row(d) + argmax[d, v]] with
    exact bf16 x fp32 products -- equal to a float64 evaluation up to fp32 summation; every width the kernel is instantiated for,
    group tails (B not a multiple of 64 / RPW), vocabulary tails, documents and rows without any gradient, accumulation into dE"""
    g = torch.Generator().manual_seed(H + B)
    if ragged:
        lens = (torch.randint(1, S // 16 + 1, (B,), generator=g) * 16).tolist()
        _, off_np, rows, row_doc, pos, _ = _ragged(lens)
        rag = ops.Ragged(dev(off_np.astype(np.int32)), dev(row_doc[::16].astype(np.int32)), dev(pos.astype(np.int32)), rows, B, S)
        off = off_np.tolist()
    else:
        lens, off, rag = [S] * B, [i * S for i in range(B + 1)], None
    T = off[-1]
    t = torch.randn(T, H, generator=g).to(torch.bfloat16)
    rep = torch.rand(B, V, generator=g) + 0.05
    rep[torch.rand(B, V, generator=g) < 0.4] = 0.0
    rep[B // 2] = 0.0                     # a document without any gradient
    rep[:, V // 3] = 0.0                  # a vocabulary row without any gradient
    grad = torch.randn(B, V, generator=g)
    am = torch.stack([torch.randint(0, lens[b], (V,), generator=g) for b in range(B)]).to(torch.int16)
    dE0 = torch.randn(V, H, generator=g)
    db0 = torch.randn(V, generator=g)
    dE, db = dev(dE0.clone()), dev(db0.clone())
    ops.sparse_head_bwd(dev(grad), dev(rep), dev(am).view(torch.uint16), dev(t, torch.bfloat16), None, dE, db, B, S, V, False, rag, part="de")
    gr = (grad.double() * torch.where(rep > 0, torch.exp(-rep.double()), torch.zeros(B, V, dtype=torch.float64)))
    want = dE0.double()
    for b in range(B):
        want += gr[b][:, None] * t[off[b] + am[b].long()].double()
    scale = float(want.abs().max())
    assert float((dE.cpu().double() - want).abs().max()) <= 2e-6 * scale
    wb = db0.double() + gr.sum(0)
    assert float((db.cpu().double() - wb).abs().max()) <= 2e-6 * float(wb.abs().max())


def test_head_de_row_gathers_random_shapes(ops):
    """property test (hypothesis): random document counts, lengths, vocabulary sizes, live-entry densities and widths -- the
    row-gather dE kernel equals the float64 routed sum, and untouched rows of dE / dbias keep their values"""
    from hypothesis import given, settings, strategies as st, HealthCheck

    @settings(max_examples=30, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(B=st.integers(1, 70), S16=st.integers(1, 8), V=st.integers(2, 1500), H=st.sampled_from([128, 256, 384, 512, 768, 1024]),
           dens=st.sampled_from([0.0, 0.02, 0.5, 1.0]), l0=st.booleans(), seed=st.integers(0, 2 ** 16))
    def run(B, S16, V, H, dens, l0, seed):
        S = 16 * S16
        g = torch.Generator().manual_seed(seed)
        t = torch.randn(B * S, H, generator=g).to(torch.bfloat16)
        rep = (torch.rand(B, V, generator=g) + 0.05) * (torch.rand(B, V, generator=g) < dens)
        grad = torch.randn(B, V, generator=g)
        am = torch.randint(0, S, (B, V), generator=g).to(torch.int16)
        dE0, db0 = torch.randn(V, H, generator=g), torch.randn(V, generator=g)
        dE, db = dev(dE0.clone()), dev(db0.clone())
        ops.sparse_head_bwd(dev(grad), dev(rep), dev(am).view(torch.uint16), dev(t, torch.bfloat16), None, dE, db, B, S, V, l0, None, part="de")
        r = rep.double()
        fp = torch.where(rep > 0, torch.exp(-r - torch.expm1(r)) if l0 else torch.exp(-r), torch.zeros_like(r))
        gr = grad.double() * fp
        want = dE0.double()
        rows = torch.arange(B)[:, None] * S + am.long()
        for b in range(B):
            want += gr[b][:, None] * t[rows[b]].double()
        wb = db0.double() + gr.sum(0)
        assert float((dE.cpu().double() - want).abs().max()) <= 3e-6 * (1 + float(want.abs().max()))
        assert float((db.cpu().double() - wb).abs().max()) <= 3e-6 * (1 + float(wb.abs().max()))

    run()


def test_prune_rows(ops):
    rep = torch.relu(rnd(7, 333, seed=1))
    out = ops.prune_rows(dev(rep.clone()), 0.1)
    mx = rep.max(-1)[0].unsqueeze(1) * 0.1
    assert torch.equal(out.cpu(), rep * (rep > mx))


# ------------------------------------------------------------------ [B,V] kernels vs golden vectors
def test_inf_free_golden(ops):
    g = np.load(os.path.join(GOLDEN, "g2_inf_free.npz"))
    ids, idf = dev(g["input_ids"]), dev(g["idf_vector"])
    special = dev(g["special_token_ids"].astype(np.int32))
    out = ops.inf_free_fwd(ids, idf, special)
    assert np.array_equal(out.cpu().numpy(), g["rep"])
    up = rnd(*g["rep"].shape, seed=1)
    gi = torch.zeros_like(idf)
    ops.inf_free_bwd(ids, idf, special, dev(up), gi)
    idf_r = torch.tensor(g["idf_vector"], requires_grad=True)
    (O.encode_inf_free(torch.tensor(g["input_ids"]), idf_r, g["special_token_ids"].tolist()) * up).sum().backward()
    close(gi, idf_r.grad, 1e-6, "idf grad")


def test_flops_golden(ops):
    g = np.load(os.path.join(GOLDEN, "g3_flops.npz"))
    rep = dev(g["rep"])
    for thr in (None, 8, 14):
        for grp in (3, 1):
            val, colmean, rowkeep = ops.flops_fwd(rep, grp, thr)
            close(val.reshape(()), torch.tensor(g[f"value_thr{thr}_g{grp}"]), 1e-5, f"value thr={thr} g={grp}")
            grad = torch.zeros_like(rep)
            ops.flops_bwd(rep, colmean, rowkeep, torch.ones(1, device="cuda"), grp, 0, rep.shape[0], grad, False)
            close(grad, torch.tensor(g[f"grad_thr{thr}_g{grp}"]), 1e-5, f"grad thr={thr} g={grp}")
            part = torch.zeros(4, rep.shape[1], device="cuda")
            ops.flops_bwd(rep, colmean, rowkeep, torch.full((1,), 0.5, device="cuda"), grp, 3, 4, part, False)
            close(part, 0.5 * torch.tensor(g[f"grad_thr{thr}_g{grp}"])[3:7], 1e-5, "local slice")


def test_losses_golden(ops):
    g = np.load(os.path.join(GOLDEN, "g4_losses.npz"))
    qd, dd_ = dev(g["q"]), dev(g["d"])
    nq, k = g["q"].shape[0], g["d"].shape[0] // g["q"].shape[0]
    for tag in [t[len("value_"):] for t in g.files if t.startswith("value_")]:
        name, ibn, tau, w = tag.split("_")
        ibn, tau, w = ibn == "ibn1", float(tau[1:]), float(w[1:])
        pairs = not ibn
        teacher = dev(g["scores_ibn"] if ibn else g["scores"])
        if name == "infonce":
            s = ops.scores_fwd(qd, dd_, pairs)
            loss, ds = ops.infonce(s, k, pairs)
        else:
            s = ops.scores_fwd(qd, dd_, pairs)
            loss, ds = (ops.kldiv if name == "kldiv" else ops.marginmse)(s, teacher, tau)
        close(w * loss.reshape(()), torch.tensor(g["value_" + tag]), 1e-5, "loss " + tag)
        dq, ddoc = torch.zeros_like(qd), torch.zeros_like(dd_)
        ops.scores_bwd(qd, dd_, ds, pairs, dq, ddoc, False)
        close(w * dq, torch.tensor(g["gq_" + tag]), 1e-4, "dq " + tag)
        close(w * ddoc, torch.tensor(g["gd_" + tag]), 1e-4, "dd " + tag)


def test_scores_large_shapes(ops):
    nq, k, D = 9, 5, 30522
    qv = torch.relu(rnd(nq, D, seed=1) - 1.5)
    dv = torch.relu(rnd(nq * k, D, seed=2) - 1.0)
    close(ops.scores_fwd(dev(qv), dev(dv), False), qv @ dv.t(), 1e-4, "all pairs")
    close(ops.scores_fwd(dev(qv), dev(dv), True), torch.einsum("bkv,bv->bk", dv.view(nq, k, D), qv), 1e-4, "pairs")
    ds = rnd(nq, nq * k, seed=3)
    dq, dd_ = torch.zeros(nq, D, device="cuda"), torch.zeros(nq * k, D, device="cuda")
    ops.scores_bwd(dev(qv), dev(dv), dev(ds), False, dq, dd_, False)
    close(dq, ds @ dv, 1e-4, "dq")
    close(dd_, ds.t() @ qv, 1e-4, "dd")


def test_teacher_ensemble_golden(ops):
    g = np.load(os.path.join(GOLDEN, "g5_teacher.npz"))
    for ibn in (0, 1):
        acc = None
        for i in range(2):
            s = ops.scores_fwd(dev(g[f"q{i}_ibn{ibn}"]), dev(g[f"d{i}_ibn{ibn}"]), not ibn)
            if acc is None:
                acc = torch.empty_like(s)
            ops.minmax_accumulate(s, 30.0 / 2, acc, i > 0)
        close(acc, torch.tensor(g[f"scores_ibn{ibn}"]), 1e-5, f"ensemble ibn={ibn}")


def test_adamw_matches_torch(ops):
    n = 10007
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2) * 0.1
    n_pad = (n + 3) // 4 * 4
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=1e-3, weight_decay=0.01)
    p = dev(torch.cat([p0, torch.zeros(n_pad - n)]))[:n]
    m, v = torch.zeros(n_pad, device="cuda")[:n], torch.zeros(n_pad, device="cuda")[:n]
    for step in range(1, 4):
        grad = g0 * step
        pt.grad = grad.clone()
        opt.step()
        ops.adamw(p, dev(grad), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step)
    close(p, pt.detach(), 1e-6, "params after 3 steps")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_weight(ops, dtype):
    w = rnd(70, 45, seed=1)
    out = torch.zeros(72, 48, dtype=dtype, device="cuda")
    out_t = torch.zeros(45, 72, dtype=dtype, device="cuda")
    ops.cast_weight(dev(w), out, out_t)
    assert torch.equal(out[:70, :45].cpu(), w.to(dtype))
    assert torch.equal(out_t[:, :70].cpu(), w.t().to(dtype))
    assert out[70:].abs().sum() == 0


@pytest.mark.parametrize("pairs", [False, True])
def test_sparse_query_scores_match_dense(ops, pairs):
    """inference-free queries: row compaction + gather-dot kernels == the dense score kernels"""
    nq, k, V, cap = 7, 4, 30522, 32
    g = torch.Generator().manual_seed(3)
    qv = torch.zeros(nq, V)
    for i in range(nq):
        n = int(torch.randint(0, cap + 1, (1,), generator=g)) if i else cap  # row 0 full, some rows empty-ish
        idx = torch.randperm(V, generator=g)[:n]
        qv[i, idx] = torch.rand(n, generator=g) * 5 + 0.1
    dv = torch.relu(rnd(nq * k, V, seed=2) - 0.5)
    csr = ops.row_compact(dev(qv), cap)
    assert int(csr[3].item()) == 0
    assert torch.equal(csr[2].cpu(), (qv != 0).sum(1).int())
    s_sparse = ops.scores_csr_fwd(csr, dev(dv), pairs)
    s_dense = ops.scores_fwd(dev(qv), dev(dv), pairs)
    close(s_sparse, s_dense, 1e-5, "scores")
    ref = torch.einsum("bkv,bv->bk", dv.view(nq, k, V), qv) if pairs else qv @ dv.t()
    close(s_sparse, ref, 1e-4, "scores vs torch")
    ds = rnd(*ref.shape, seed=4)
    dq, dd_ = torch.empty(nq, V, device="cuda"), torch.empty(nq * k, V, device="cuda")
    ops.scores_csr_bwd(csr, dev(dv), dev(ds), pairs, dq, dd_)
    if pairs:
        dd_ref = (ds[:, :, None] * qv[:, None, :]).reshape(nq * k, V)
        dq_ref = torch.einsum("bk,bkv->bv", ds, dv.view(nq, k, V))
    else:
        dd_ref, dq_ref = ds.t() @ qv, ds @ dv
    close(dd_, dd_ref, 1e-4, "dd")
    close(dq, dq_ref * (qv != 0), 1e-4, "dq (restricted to q's support)")
    over = ops.row_compact(dev(qv), 8)
    assert int(over[3].item()) > 0, "rows with more than cap non-zeros must be flagged"


def _ragged(lens):
    """host-side packing metadata exactly as sparse_hip.encoder.pack_documents builds it"""
    lens = np.asarray(lens)
    L16 = (lens + 15) // 16 * 16
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(L16, out=off[1:])
    rows = int(off[-1])
    row_doc = np.repeat(np.arange(len(lens)), L16)
    pos = np.arange(rows) - np.repeat(off[:-1], L16)
    return lens, off, rows, row_doc, pos, pos < lens[row_doc]


@pytest.mark.parametrize("dtype,H", [(torch.float32, 128), (torch.bfloat16, 128), (torch.bfloat16, 384)])
@pytest.mark.parametrize("use_l0", [False, True])
def test_sparse_head_ragged_layout(ops, dtype, H, use_l0):
    """un-padded documents (each a multiple of 16 rows, spanning row tiles arbitrarily): the fused head
    and its backward must equal the per-document dense computation"""
    lens, off, rows, row_doc, pos, valid = _ragged([37, 128, 16, 90, 5, 64, 100, 128, 77, 3, 250, 512, 300])
    B, V = len(lens), 700
    rag = ops.Ragged(dev(off.astype(np.int32)), dev(row_doc[::16].astype(np.int32)), dev(pos.astype(np.int32)), rows, B, 512)
    t = q(rnd(rows, H, seed=1), dtype)
    E = q(rnd(V, H, seed=2, scale=0.3 if H < 384 else 0.15), dtype)
    bias = rnd(V, seed=3, scale=0.5)
    mask = torch.from_numpy(valid.astype(np.uint8))
    rep, am = ops.sparse_head_fwd(dev(t, dtype), dev(E, dtype), dev(bias), dev(mask), B, 512, V, use_l0, rag)
    tr, Er, br = t.clone().requires_grad_(True), E.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    refs, tops, lgs = [], [], []
    for b in range(B):
        lg = tr[off[b]:off[b] + lens[b]] @ Er.t() + br
        refs.append(O.sparse_activation(lg[None], torch.ones(1, int(lens[b]), dtype=torch.long), use_l0)[0])
        tops.append(lg.detach())
        lgs.append(lg)
    ref = torch.stack(refs)
    tol = TOL[dtype] * 2
    close(rep, ref, tol, "rep")
    posn = am.cpu().long() & 0xFFFF
    for b in range(B):
        live = ref[b] > 0
        # (documents of 3 and 5 tokens: their padded rows are copies of row 0 inside the device's stage -- a NEGATIVE raw maximum on
        #  row 0 must not come out at the copy in position 7; round 6 found exactly that in the vocabulary-stationary kernels)
        assert (posn[b][live] < int(lens[b])).all(), (b, int(lens[b]), posn[b][live & (posn[b] >= int(lens[b]))][:8])
        picked = tops[b].gather(0, posn[b].clamp(max=int(lens[b]) - 1)[None])[0]
        top = tops[b].max(0).values
        assert (picked[live] >= top[live] - (1e-4 if dtype == torch.float32 else 2.0 ** -12 * (top[live].abs() + br.detach().abs().max() + 1))).all()
    up = rnd(B, V, seed=4)
    if dtype != torch.float32:  # gradients flow to the position the device chose among near-ties (inside the window asserted above)
        ref = torch.stack([O.sparse_activation(lgs[b][None], torch.ones(1, int(lens[b]), dtype=torch.long), use_l0,
                                               route=posn[b].clamp(max=int(lens[b]) - 1)[None])[0] for b in range(B)])
    (ref * up).sum().backward()
    dE, dbias = torch.zeros(V, H, device="cuda"), torch.zeros(V, device="cuda")
    dt = ops.sparse_head_bwd(dev(up), rep, am, dev(t, dtype), dev(E, dtype), dE, dbias, B, 512, V, use_l0, rag)
    want_dt = tr.grad.clone()
    want_dt[~torch.from_numpy(valid)] = 0
    close(dt, want_dt, tol * 2, "dt")
    close(dE, Er.grad, tol * 2, "dE")
    close(dbias, br.grad, tol * 2, "dbias")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("A,dh,S,doc_lens", [(2, 32, 128, [37, 128, 16, 90, 5, 64]), (3, 64, 512, [300, 512, 17, 129, 480, 64, 255]),
                                             (2, 64, 256, [256, 100, 31]), (3, 32, 512, [511, 48, 200])])
def test_attention_ragged_layout(ops, dtype, A, dh, S, doc_lens):
    """un-padded documents against the per-document eager attention.  What launch_fwd / launch_bwd pick for these rows in bf16 (the
    table of tests/test_attention_gpu.py): (2, 32, 128) 4 waves forward and attn_bwd1_kernel; (2, 64, 256) 8 waves forward, the two-phase
    backward with 12; (3, 64, 512) (configs[4]: head dim 64, up to 512 tokens) and (3, 32, 512) (unpaired heads) the two-group forward with
    16 waves and the two-phase backward with 12.  fp32 parity mode: 4 waves everywhere"""
    if dtype == torch.float32 and S * dh > 256 * 64:
        pytest.skip("fp32 parity mode: two [S][dh] fp32 LDS images cap S*dh at 256*64")
    lens, off, rows, row_doc, pos, valid = _ragged(doc_lens)
    B = len(lens)
    H = A * dh
    rag = ops.Ragged(dev(off.astype(np.int32)), dev(row_doc[::16].astype(np.int32)), dev(pos.astype(np.int32)), rows, B, S)
    qkv = q(rnd(rows, 3 * H, seed=1), dtype)
    dctx = q(rnd(rows, H, seed=2), dtype)
    mask = torch.from_numpy(valid.astype(np.uint8))
    ctx, lse = ops.attention_fwd(dev(qkv, dtype), dev(mask), B, S, A, None, rag)
    xr = qkv.clone().requires_grad_(True)
    want = torch.zeros(rows, H)
    for b in range(B):
        n = int(lens[b])
        cr, _ = ref_attention(xr[off[b]:off[b] + n], torch.ones(1, n), 1, n, A, dh)
        want[off[b]:off[b] + n] = cr
    tol = TOL[dtype] * 2
    vm = torch.from_numpy(valid)
    close(ctx.float().cpu()[vm], want.detach()[vm], tol, "ctx")
    (want * dctx).sum().backward()
    dqkv = ops.attention_bwd(dev(qkv, dtype), dev(mask), ctx, dev(dctx * vm[:, None], dtype), lse, B, S, A, None, rag)
    close(dqkv.float().cpu()[vm], xr.grad[vm], tol * 2, "dqkv")


# ------------------------------------------------------------------ fp16 forward operands of a bf16 run (SM_F16)
@pytest.mark.parametrize("M,N,K", [(200, 136, 128), (6151, 1152, 384), (4100, 384, 1536), (49200, 768, 1024), (6200, 384, 1024)])
def test_gemm_nt_fp16_operands(ops, M, N, K):
    """fp16 A / B: C fp16 (or fp32 with out_f32), the pre-activation copy stays bf16; against the fp32 product of the fp16-rounded
    operands: 2e-3 of the scale (the bf16 form of the same test asserts 2e-2)"""
    h = torch.float16
    A, B = q(rnd(M, K, seed=1, scale=0.5), h), q(rnd(N, K, seed=2, scale=0.5), h)
    bias = rnd(N, seed=3)
    ref = A @ B.t() + bias
    pre = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    out = ops.gemm_nt(dev(A, h), dev(B, h), bias=dev(bias), act=1, preact=pre)
    assert out.dtype == h
    close(pre, ref, 1e-2, "pre-activation (bf16 storage)")
    close(out, O._gelu(ref), 2e-3, "gelu (fp16)")
    res = rnd(M, N, seed=4)
    out32 = ops.gemm_nt(dev(A, h), dev(B, h), bias=dev(bias), residual=dev(res), out_f32=True)
    assert out32.dtype == torch.float32
    close(out32, ref + res, 2e-3, "fp32 out + fp32 residual")


def test_gemm_nt_gelu_out(ops):
    """backward of FFN-down with the post-GELU tensor re-created in the same epilogue (hf:336 backward)"""
    M, N, K = 4100, 1536, 384
    bf = torch.bfloat16
    A, B, x = q(rnd(M, K, seed=1, scale=0.3), bf), q(rnd(N, K, seed=2, scale=0.3), bf), q(rnd(M, N, seed=3), bf)
    ga = torch.empty(M, N, dtype=bf, device="cuda")
    out = ops.gemm_nt(dev(A, bf), dev(B, bf), gelu_grad_of=dev(x, bf), gelu_out=ga)
    plain = ops.gemm_nt(dev(A, bf), dev(B, bf), gelu_grad_of=dev(x, bf))
    assert torch.equal(out, plain)
    close(ga, O._gelu(x), 1e-2, "gelu_out")


@pytest.mark.parametrize("B,S,H,V,rag_mode", [(6, 64, 384, 3000, "dense"), (5, 128, 768, 2500, "dense"), (3, 512, 128, 1500, "dense")])
def test_sparse_head_fwd_fp16_operands(ops, B, S, H, V, rag_mode):
    """t, E in fp16 (the narrow vocabulary-stationary kernel at H = 384 and, with 9 position bits, at H = 128 / S = 512; the wide one
    at H = 768): against fp32 on the same fp16-rounded operands 2e-3 of the scale; the arg-max is a position inside the document
    that attains the maximum within the window of tests/test_head_fwd_gpu.py (fp64 logits; never wider than the 1e-2 asserted
    before)"""
    h = torch.float16
    t = q(rnd(B * S, H, seed=1), h)
    E = q(rnd(V, H, seed=2, scale=0.3), h)
    bias = rnd(V, seed=3, scale=0.5)
    mask = torch.ones(B, S, dtype=torch.uint8)
    for b in range(1, B):
        mask[b, S - 3 * b - 2:] = 0
    Epad = torch.zeros((V + 127) // 128 * 128, H)
    Epad[:V] = E
    rep, am = ops.sparse_head_fwd(dev(t, h), dev(Epad, h), dev(bias), dev(mask), B, S, V, False)
    logits = (t @ E.t() + bias).view(B, S, V)
    ref = O.sparse_activation(logits, mask.long(), False)
    close(rep, ref, 2e-3, "rep (fp16 operands)")
    pos = am.cpu().long() & 0xFFFF
    live = ref > 0
    lens = mask.long().sum(1)[:, None]
    assert (pos < lens)[live].all(), "an arg-max position outside its document"
    # fp64 logits of the same operands; value bound = truncation to the position bits + worst-case fp32 accumulation + v_log_f32
    attended = mask[:, :, None] != 0
    raw64 = (t.double() @ E.double().t()).view(B, S, V).masked_fill(~attended, -float("inf"))
    A = (t.double().abs() @ E.double().abs().t()).view(B, S, V).masked_fill(~attended, 0).max(1).values
    picked = torch.gather(raw64, 1, pos[:, None, :]).squeeze(1)
    top = raw64.max(1).values
    idx_mask = 15
    while idx_mask < S - 1:
        idx_mask = idx_mask * 2 + 1
    bound = 2.0 ** -(23 - idx_mask.bit_length()) * top.abs() + 2 * H * 2.0 ** -24 * A + 1e-6
    window = torch.minimum(2 * bound, 2.0 ** -12 * ((top + bias.double()).abs() + float(bias.abs().max()) + 1)).clamp(max=1e-2)
    assert (picked[live] >= (top - window)[live]).all()


def test_layernorm_res32_fp16_copy(ops):
    rows, H = 1000, 768
    x = rnd(rows, H, seed=1) * 2 + 0.3
    gamma, beta = 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)
    y, y32, mean, rstd, y16 = ops.layernorm_fwd_res32(dev(x), dev(gamma), dev(beta), 1e-12, torch.bfloat16, want_y32=True, want_y16=True)
    assert y16.dtype == torch.float16 and torch.equal(y16, y32.to(torch.float16)) and torch.equal(y, y32.to(torch.bfloat16))
    close(y32, O._ln(x, gamma, beta, 1e-12), 1e-5, "fp32 output")


# ---- fp8 operands (BASELINE configs[4]; csrc/fp8.hip, sm_gemm_nt SM_FP8 / SM_FP8_GRAD) ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("e5m2", [False, True])
def test_quantize_fp8_matches_the_torch_conversion(ops, dtype, e5m2):
    """per-tensor scaling: q = fp8(x * fmax / amax) byte for byte what torch's CPU round-to-nearest-even conversion gives (OCP
    e4m3fn / e5m2), scale = amax / fmax; also the odd tail (n % 8 != 0) and a tensor whose amax sits in the tail"""
    g = torch.Generator(device="cuda").manual_seed(3)
    for n in (8 * 4096 + 5, 1237, 64):
        x = (torch.randn(n, device="cuda", generator=g) * 3).to(dtype)
        x[-1] = 17.5
        q, scale, amax = ops.quantize_fp8(x, e5m2=e5m2)
        fmax = 57344.0 if e5m2 else 448.0
        assert float(amax) == 17.5 and abs(float(scale) - 17.5 / fmax) < 1e-9
        ref = (x.float().cpu() * (torch.tensor(fmax) / torch.tensor(17.5))).clamp(-fmax, fmax).to(torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn)
        assert torch.equal(q.cpu().view(torch.uint8), ref.view(torch.uint8))
        # delayed scaling: scale from a given (stale, here smaller) maximum taken with a margin of 2 (a tensor may double from one
        # step to the next), values past it saturate; this pass's maximum is recorded
        stale, nxt = torch.full((1,), 4.0, device="cuda"), torch.zeros(1, device="cuda")
        q2, scale2, _ = ops.quantize_fp8(x, e5m2=e5m2, amax=stale, amax_next=nxt)
        assert float(nxt) == 17.5 and abs(float(scale2) - 8.0 / fmax) < 1e-9
        ref2 = (x.float().cpu() * (torch.tensor(fmax) / torch.tensor(8.0))).clamp(-fmax, fmax).to(torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn)
        assert torch.equal(q2.cpu().view(torch.uint8), ref2.view(torch.uint8))
    # a non-finite element is NOT laundered into a finite value: the measured maximum is NaN, the scale derived from it is NaN (the GEMM
    # multiplies by the scale), and under delayed scaling the recorded maximum is NaN so the NEXT step's scale is
    for poison in (float("nan"), float("inf")):
        x = (torch.randn(4099, device="cuda", generator=g) * 3).to(dtype)
        x[1234] = poison
        q, scale, amax = ops.quantize_fp8(x, e5m2=e5m2)
        assert float(amax) != float(amax) and float(scale) != float(scale)
        nxt = torch.zeros(1, device="cuda")
        ops.quantize_fp8(x, e5m2=e5m2, amax=torch.full((1,), 4.0, device="cuda"), amax_next=nxt)
        assert float(nxt) != float(nxt)
        _, scale3, _ = ops.quantize_fp8(torch.ones(64, device="cuda", dtype=dtype), e5m2=e5m2, amax=nxt, amax_next=torch.zeros(1, device="cuda"))
        assert float(scale3) != float(scale3)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(1000, 3072), (77, 256), (4100, 1536)])
def test_gelu_quantize_fp8_pass_equals_its_parts(ops, rows, cols):
    """sm_gelu_quantize_fp8 (ABI 8): forward -- out16 = bf16(gelu(x)) with the bf16 epilogues' erf form (against torch's exact-erf GELU at
    bf16 rounding), q / scale / next-step maximum byte for byte what sm_quantize_fp8 (delayed scaling) gives on out16, also without the
    16-bit output; backward -- out16 = bf16(x gelu'(f1)) against the fp64 derivative, in place over x, q as sm_quantize_fp8(e5m2) of it"""
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = (torch.randn(rows, cols, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
    f1 = (torch.randn(rows, cols, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
    cur = torch.full((1,), 3.0, device="cuda")
    zero = lambda: torch.zeros(1, device="cuda")
    nxt = zero()
    ga, q, sc = ops.gelu_quantize_fp8(x, cur, nxt)
    want = torch.nn.functional.gelu(x.double())
    assert float((ga.double() - want).abs().max()) <= 2 ** -8 * float(want.abs().max()) and ga.dtype == torch.bfloat16
    nref = zero()
    q_ref, s_ref, _ = ops.quantize_fp8(ga, amax=cur, amax_next=nref)
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(sc, s_ref) and torch.equal(nxt, nref)
    n2 = zero()
    none16, q2, sc2 = ops.gelu_quantize_fp8(x, cur, n2, want16=False)
    assert none16 is None and torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(n2, nxt)
    # backward, in place
    xb = x.clone()
    n3 = zero()
    d, qd, sd = ops.gelu_quantize_fp8(xb, cur, n3, f1=f1, inplace=True)
    assert d.data_ptr() == xb.data_ptr() and qd.dtype == torch.float8_e5m2
    f = f1.double()
    gp = 0.5 * (1 + torch.erf(f / 2 ** 0.5)) + f * torch.exp(-0.5 * f * f) / (2 * torch.pi) ** 0.5
    wd = x.double() * gp
    assert float((d.double() - wd).abs().max()) <= 2 ** -7 * float(wd.abs().max())
    n4 = zero()
    qd_ref, sd_ref, _ = ops.quantize_fp8(d, e5m2=True, amax=cur, amax_next=n4)
    assert torch.equal(qd.view(torch.uint8), qd_ref.view(torch.uint8)) and torch.equal(sd, sd_ref) and torch.equal(n3, n4)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(200, 136, 128), (4100, 768, 768), (2100, 3072, 768), (1000, 768, 3072)])
@pytest.mark.parametrize("grad", [False, True])
def test_gemm_nt_fp8_operands(ops, M, N, K, grad):
    """C = (qA . qB^T) * sa * sb: against the same product of the DEQUANTISED operands in fp64 (the fp8 MFMA multiplies exactly and
    accumulates in fp32), fp32 output 1e-4, bf16 output at its rounding; forward (e4m3 x e4m3) and input-gradient (e5m2 x e4m3)
    formats, with the bias / GELU / pre-activation / residual epilogue of the encoder linears"""
    g = torch.Generator(device="cuda").manual_seed(1)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.7).to(torch.bfloat16)
    b = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    qa, sa, _ = ops.quantize_fp8(a, e5m2=grad)
    qb, sb, _ = ops.quantize_fp8(b)
    want = (qa.float().double() @ qb.float().double().t()) * float(sa) * float(sb)
    got32 = ops.gemm_nt(qa, qb, scale_a=sa, scale_b=sb, out_f32=True)
    scale = want.abs().max()
    assert float((got32.double() - want).abs().max() / scale) < 1e-4  # (fp32 accumulation inside and between the MFMAs)
    got = ops.gemm_nt(qa, qb, scale_a=sa, scale_b=sb)
    assert got.dtype == torch.bfloat16 and float((got.double() - want).abs().max() / scale) < 5e-3
    # and the quantisation error itself against the bf16 operands (what the fp8 format costs): printed, loosely bounded
    exact = a.double() @ b.double().t()
    rel = float((want - exact).norm() / exact.norm())
    print(f"[fp8 gemm {M}x{N}x{K} {'e5m2' if grad else 'e4m3'} x e4m3] relative Frobenius error of the product {rel:.3e}")
    assert rel < (1.5e-1 if grad else 6e-2)
    if not grad:  # the encoder's forward epilogue: bias + GELU with the pre-activation kept, and an fp32 residual
        bias = torch.randn(N, device="cuda", generator=g) * 0.1
        pre = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        act = ops.gemm_nt(qa, qb, bias=bias, act=1, preact=pre, scale_a=sa, scale_b=sb)
        wpre = want + bias.double()
        assert float((pre.double() - wpre).abs().max() / scale) < 5e-3
        assert float((act.double() - torch.nn.functional.gelu(wpre)).abs().max() / scale) < 6e-3
        res = torch.randn(M, N, device="cuda", generator=g)
        z = ops.gemm_nt(qa, qb, bias=bias, residual=res, out_f32=True, scale_a=sa, scale_b=sb)
        assert float((z.double() - (wpre + res.double())).abs().max() / (scale + 4)) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,fp8_in", [(4100, 3072, 768, True), (2100, 768, 768, True), (1000, 1152, 384, False), (130, 136, 128, True)])
@pytest.mark.parametrize("e5m2", [False, True])
def test_gemm_nt_epilogue_emits_the_next_gemms_fp8_operand(ops, M, N, K, fp8_in, e5m2):
    """sm_epilogue.q8 (ABI 6): the epilogue writes its result as fp8 with sm_quantize_fp8's arithmetic on the 16-bit value it stores --
    the SAME bytes, scale and next-step maximum as a separate sm_quantize_fp8 pass over the stored tensor (delayed scaling: the
    scale comes from an earlier maximum, here half and twice the true one: saturation and head room); with and without the 16-bit
    output; fp8 and bf16 operands; the FFN-up epilogue (bias + GELU + pre-activation)"""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.7).to(torch.bfloat16)
    b = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    kw = {}
    if fp8_in:
        qa, sa, _ = ops.quantize_fp8(a)
        qb, sb, _ = ops.quantize_fp8(b)
        A, B, kw = qa, qb, dict(scale_a=sa, scale_b=sb)
    else:
        A, B = a, b
    pre = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    ref = ops.gemm_nt(A, B, bias=bias, act=1, preact=pre, **kw)
    true_max = ref.float().abs().max().reshape(1)
    for factor in (0.5, 2.0):
        cur = true_max * factor
        nxt_ref = torch.full((1,), 0.01, device="cuda")
        q_ref, s_ref, _ = ops.quantize_fp8(ref, e5m2=e5m2, amax=cur, amax_next=nxt_ref)
        for no_out in (False, True):
            nxt = torch.full((1,), 0.01, device="cuda")
            pre2 = torch.empty_like(pre)
            out, q, s = ops.gemm_nt(A, B, bias=bias, act=1, preact=pre2, q8=(cur, nxt, e5m2), no_out=no_out, **kw)
            assert (out is None) == no_out and (no_out or torch.equal(out, ref)) and torch.equal(pre2, pre)
            assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)), "fp8 bytes differ from a separate quantisation pass"
            assert float(s) == float(s_ref) and float(nxt) == float(nxt_ref) == float(true_max)
    # a non-finite value in the result poisons the next step's maximum exactly as the separate pass does
    bias_bad = bias.clone()
    bias_bad[3] = float("inf")
    nxt = torch.zeros(1, device="cuda")
    ops.gemm_nt(A, B, bias=bias_bad, q8=(true_max, nxt, e5m2), **kw)
    assert float(nxt) != float(nxt)


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nd", [(256, 1024), (70, 333), (32, 512)])
def test_scores_on_the_matrix_pipe(ops, nq, nd):
    """all-pairs score matrix and its backward for DENSE queries through the fp32-MFMA kernels (csrc/scores_mfma.hip: split over
    V with fp32 atomics / NN form), V = 30522 (rows 8-byte aligned only, tail of 26 columns): against fp64 products at 1e-4 of the
    largest element -- loss.py:33-37, :94-98"""
    D = 30522
    g = torch.Generator(device="cuda").manual_seed(nq)
    q = torch.relu(torch.randn(nq, D, device="cuda", generator=g) - 1.0)
    d = torch.relu(torch.randn(nd, D, device="cuda", generator=g) - 0.5)
    s = ops.scores_fwd(q, d, False)
    want = q.double() @ d.double().t()
    assert float((s.double() - want).abs().max() / want.abs().max()) < 1e-4
    ds = torch.randn(nq, nd, device="cuda", generator=g)
    dq, dd_ = torch.zeros(nq, D, device="cuda"), torch.full((nd, D), 0.5, device="cuda")
    ops.scores_bwd(q, d, ds, False, dq, None, False)
    ops.scores_bwd(q, d, ds, False, None, dd_, True)   # accumulate into 0.5
    wq, wd = ds.double() @ d.double(), ds.double().t() @ q.double() + 0.5
    assert float((dq.double() - wq).abs().max() / wq.abs().max()) < 1e-4
    assert float((dd_.double() - wd).abs().max() / wd.abs().max()) < 1e-4
    # deterministic form (one split of V, no atomics): the same matrix bit for bit on every launch
    s1, s2 = ops.scores_fwd(q, d, False, deterministic=True), ops.scores_fwd(q, d, False, deterministic=True)
    assert torch.equal(s1, s2)
    assert float((s1.double() - want).abs().max() / want.abs().max()) < 1e-4


# ---- weight-stationary NT GEMM for K = 384 (csrc/gemm_ws.hip) ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,bias", [(8192, 1152, True), (43904 + 16, 384, False), (12345 // 16 * 16, 1536, True), (65536, 1152, True),
                                      (8200 + 9, 128, True), (9001, 2048, False)])  # (rows that are no multiple of 16 / 32; one and sixteen column slices)
def test_gemm_ws_plain_epilogue(ops, M, N, bias):
    """C = A . W^T (+ bias) at K = 384, M >= 8192 through the weight-stationary kernel: against the fp64 product at bf16 rounding, and
    against the 128 x 128 kernel (taken below 8192 rows) on the first and last rows -- same products, different summation order"""
    g = torch.Generator(device="cuda").manual_seed(M % 1000)
    a = (torch.randn(M, 384, device="cuda", generator=g) * 0.7).to(torch.bfloat16)
    w = (torch.randn(N, 384, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, device="cuda", generator=g) * 0.1 if bias else None
    got = ops.gemm_nt(a, w, bias=b)
    torch.cuda.synchronize()
    for sl in (slice(0, 4096), slice(M - 4096, M), slice(M // 2 - 1000, M // 2 + 1000)):
        want = a[sl].double() @ w.double().t() + (b.double() if bias else 0)
        err = (got[sl].double() - want).abs()
        assert float((err / (want.abs() * 2 ** -7 + 2e-3)).max()) <= 1.0, float(err.max())
        old = ops.gemm_nt(a[sl].contiguous(), w, bias=b)
        assert float((old.float() - got[sl].float()).abs().max()) <= 2 ** -6 * float(want.abs().max())
    again = ops.gemm_nt(a, w, bias=b)
    assert torch.equal(got, again), "two launches on the same inputs must agree bit for bit"


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,bias", [(8192, 2304, True), (8192 + 300 + 9, 768, False), (20000, 768, True), (65536, 128, True)])
@pytest.mark.parametrize("grad", [False, True])
def test_gemm_ws_fp8_plain_epilogue(ops, M, N, bias, grad):
    """round 6: C = (qA . qW^T) sa sb (+ bias) at K = 768, M >= 8192 on fp8 operands through the weight-stationary kernel (OPK 2: e4m3 x
    e4m3, the QKV forward; OPK 3: e5m2 x e4m3, the attention-output input gradient): against the fp64 product of the DEQUANTISED operands
    at bf16 rounding, and against the 128 x 128 fp8 kernel (taken below 8192 rows) on row slices -- the same exact products, another
    summation order; rows that end inside a 32-row step"""
    g = torch.Generator(device="cuda").manual_seed(M % 1000 + int(grad))
    a = (torch.randn(M, 768, device="cuda", generator=g) * 0.7).to(torch.bfloat16)
    w = (torch.randn(N, 768, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, device="cuda", generator=g) * 0.1 if bias else None
    qa, sa, _ = ops.quantize_fp8(a, e5m2=grad)
    qw, sw, _ = ops.quantize_fp8(w)
    got = ops.gemm_nt(qa, qw, bias=b, scale_a=sa, scale_b=sw)
    assert got.dtype == torch.bfloat16
    torch.cuda.synchronize()
    for sl in (slice(0, 4096), slice(M - 4096, M), slice(M // 2 - 1000, M // 2 + 1000)):
        want = (qa[sl].float().double() @ qw.float().double().t()) * float(sa) * float(sw) + (b.double() if bias else 0)
        err = (got[sl].double() - want).abs()
        assert float((err / (want.abs() * 2 ** -7 + 2e-3)).max()) <= 1.0, float(err.max())
        old = ops.gemm_nt(qa[sl].contiguous(), qw, bias=b, scale_a=sa, scale_b=sw)  # < 8192 rows: gemm_nt_kernel<.., fp8_op>
        assert float((old.float() - got[sl].float()).abs().max()) <= 2 ** -6 * float(want.abs().max())
    again = ops.gemm_nt(qa, qw, bias=b, scale_a=sa, scale_b=sw)
    assert torch.equal(got, again), "two launches on the same inputs must agree bit for bit"


@pytest.mark.gpu
@pytest.mark.parametrize("M", [8192, 8300])
@pytest.mark.parametrize("with_ln", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gemm_ws_fp8_fp32_residual_epilogue(ops, M, with_ln, p):
    """round 6: the attention-output projection of the fp32 residual stream on fp8 operands at K = N = 768 (gemm_ws.hip, OPK 2, EPI 2):
    fp32 out = dropout((qA . qW^T) sa sb + bias) + residual (or LayerNorm of it, recomputed), against fp64 on the dequantised operands
    with the dropout mask the backward kernels regenerate"""
    from sparse_hip import lib
    dtype = torch.bfloat16
    N = K = 768
    A, B = dev(q(rnd(M, K, seed=1, scale=0.5), dtype), dtype), dev(q(rnd(N, K, seed=2, scale=0.05), dtype), dtype)
    z = rnd(M, N, seed=3, scale=1.5) + 0.2
    gamma, beta, bias = 1.0 + 0.1 * rnd(N, seed=4), 0.1 * rnd(N, seed=5), 0.1 * rnd(N, seed=6)
    zd = dev(z)
    drop = lib.dropout(p, 5, 2) if p else None
    ln = None
    res = z
    if with_ln:
        _, _, mean, rstd = ops.layernorm_fwd_res32(zd, dev(gamma), dev(beta), 1e-12, dtype)
        ln = (mean, rstd, dev(gamma), dev(beta))
        res = torch.nn.functional.layer_norm(z, (N,), gamma, beta, 1e-12)
    qa, sa, _ = ops.quantize_fp8(A)
    qb, sb, _ = ops.quantize_fp8(B)
    got = ops.gemm_nt(qa, qb, bias=dev(bias), drop=drop, residual=zd, out_f32=True, residual_ln=ln, scale_a=sa, scale_b=sb)
    lin = ((qa.float().double() @ qb.float().double().t()) * float(sa) * float(sb)).float().cpu() + bias
    if p:
        keep = ops.dropout_bwd(torch.ones(M, N, dtype=dtype, device="cuda"), drop).float().cpu() != 0
        p_q = int(p * 256 + 0.5) / 256  # the rate actually applied (include/sparse_hip.h, sm_dropout)
        lin = lin * keep / (1 - p_q)
    want = lin + res
    assert got.dtype == torch.float32
    close(got, want, 2e-5 if not with_ln else 1e-4, "fp8 fp32-residual epilogue")


@pytest.mark.gpu
@pytest.mark.parametrize("M", [8192, 43904, 20000 // 16 * 16])
def test_gemm_ws_df1_epilogue(ops, M):
    """dF1 = (dy . W2) * gelu'(f1), ga = gelu(f1) with f1 in the fused feed-forward's tile-major layout (the forward's sigmoid-form
    GELU), K = 384, N = 1536: against torch on the row-major f1"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_ffn_pc_gpu import _f1_tiles
    N = 1536
    g = torch.Generator(device="cuda").manual_seed(7)
    a = (torch.randn(M, 384, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, 384, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    f1 = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    ga = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    got = ops.gemm_nt(a, w, gelu_grad_of=_f1_tiles(f1, N), gelu_out=ga, gelu_grad_tiled=True)
    x = f1.float().requires_grad_(True)
    u = x * (1.59501576 + 7.40113008e-2 * x * x - 7.03034904e-4 * x ** 4)
    y = x * torch.sigmoid(u)
    (gp,) = torch.autograd.grad(y.sum(), x)
    want = (a.float() @ w.float().t()) * gp
    scale = float(want.abs().max())
    assert float((got.float() - want).abs().max()) <= 1.2e-2 * scale
    assert float((ga.float() - y.detach()).abs().max()) <= 2e-2 and float((ga.float() - y.detach()).abs().mean()) < 1e-3
