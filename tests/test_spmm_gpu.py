"""`spmm_kernel` (csrc/attention.hip, every GCN layer) against the float64 oracle of
tests/attention_common.py beyond the one shape of test_spmm_shared_and_flat: fp32 and bf16, the scalar
path of F % 8 != 0 (a GCN output layer has F = number of classes), the second feature trip of F > 512,
rows without edges, N % 4 != 0 (a partly filled last workgroup), a rectangular graph (Nx != N) and a
row far longer than the rest. The output buffer is filled with NaN before the launch, so a tail column
or an empty row the kernel does not write shows."""

import types

import pytest
import torch

import attention_common as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 3
DTYPES = [(torch.float32, ac.SPMM_F32_TOL), (torch.bfloat16, ac.SPMM_BF16_TOL)]
EMPTY_ROWS = (0, 17, 36)


def _csr(N, Nx, seed, long_row=5):
    """A random CSR [N, Nx] on the CPU: degrees 1-12, rows 0, 17 and 36 empty, one row of degree 150
    (columns repeat: Nx < 150), values in [0, 1). Returns (rowptr, col, val, row of every edge)."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(1, 13, (N,), generator=g)
    deg[list(EMPTY_ROWS)] = 0
    deg[long_row] = 150
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = deg.cumsum(0)
    E = int(rowptr[-1])
    col = torch.randint(0, Nx, (E,), generator=g)
    val = torch.rand(E, generator=g)
    rows = torch.repeat_interleave(torch.arange(N), deg)
    return rowptr.to(torch.int32), col.to(torch.int32), val, rows


def _transpose(rowptr, col, val, rows, Nx):
    """CSR of the transpose [Nx, N] (stable sort by column)."""
    order = torch.sort(col.long(), stable=True).indices
    rp = torch.zeros(Nx + 1, dtype=torch.int64)
    rp[1:] = torch.bincount(col.long(), minlength=Nx).cumsum(0)
    return rp.to(torch.int32), rows[order].to(torch.int32), val[order]


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [3, 7, 8, 20, 64, 515, 520])
def test_spmm_rectangular(hip, F, dtype, tol):
    N, Nx = 37, 53
    rowptr, col, val, _ = _csr(N, Nx, seed=1)
    x = torch.randn(K, Nx, F, generator=torch.Generator().manual_seed(F)).to(dtype)
    exact = ac.spmm64(rowptr, col, val, x)
    rp, cl, vl, xd = rowptr.to(DEV), col.to(DEV), val.to(DEV), x.to(DEV)
    y = torch.full((K, N, F), float("nan"), dtype=dtype, device=DEV)
    hip._C.spmm(hip._p(rp), hip._p(cl), hip._p(vl), hip._p(xd), hip._p(y), K, N, Nx, F, Nx * F, N * F,
                int(dtype == torch.float32), hip._s())
    torch.cuda.synchronize()
    assert torch.isfinite(y).all(), "an element of y was not written"
    err = ac.rel_err(y, exact)
    print(f"SPMM_ERR {'fp32' if dtype == torch.float32 else 'bf16'} F={F} {err:.3g}/{tol:.3g}")
    assert err <= tol
    assert torch.all(y[:, list(EMPTY_ROWS)] == 0), "a row without edges is not exactly 0"
    assert torch.equal(hip.spmm(rp, cl, vl, xd), y)  # the wrapper launches the same thing


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["fp32", "bf16"])
def test_spmm_autograd_square(hip, dtype, tol):
    """`functional.spmm` forward and backward (the transposed CSR) on a square graph at F = 7, against
    float64 autograd through the dense matrix."""
    from distributed_learning_simulator_amd.ops import functional as Fn

    N, F = 37, 7
    rowptr, col, val, rows = _csr(N, N, seed=2)
    rpt, clt, vlt = _transpose(rowptr, col, val, rows, N)
    graph = types.SimpleNamespace(rowptr=rowptr.to(DEV), col=col.to(DEV), val=val.to(DEV), rowptr_t=rpt.to(DEV),
                                  col_t=clt.to(DEV), val_t=vlt.to(DEV))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(K, N, F, generator=g).to(dtype)
    dy = torch.randn(K, N, F, generator=g).to(dtype)
    A = torch.zeros(N, N, dtype=torch.float64).index_put_((rows, col.long()), val.double(), accumulate=True)
    x64 = x.double().requires_grad_()
    y64 = torch.matmul(A, x64)
    (dx64,) = torch.autograd.grad(y64, x64, dy.double())
    assert ac.rel_err(y64, ac.spmm64(rowptr, col, val, x)) < 1e-14  # the two oracles agree
    xd = x.to(DEV).requires_grad_()
    y = Fn.spmm(xd, graph)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    ey, ex = ac.rel_err(y, y64), ac.rel_err(xd.grad, dx64)
    print(f"SPMM_ERR {'fp32' if dtype == torch.float32 else 'bf16'} autograd y={ey:.3g} dx={ex:.3g} /{tol:.3g}")
    assert ey <= tol and ex <= tol
