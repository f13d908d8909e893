"""Plain float64 restatements of the linear kernels, for the rounding bound of test_gpu_variants and test_gpu_fuzz.

The bound: |got - ref64| <= c * 2^-24 * ref_abs + TINY per output, where ref_abs is the same restatement over absolute
values (the sum of |terms| of that output) and c is a per-operator constant stated next to each use (<= 32).  2^-24 is
the unit roundoff of fp32; a kernel that adds the right terms in any order stays well inside c of it, a kernel that drops
one term or reads a neighbour one pixel off does not (the CPU self-checks in test_gpu_variants plant exactly those)."""
import torch

U32 = 2.0 ** -24
TINY = 2.0 ** -120


def violations(got, ref, ref_abs, c):
    """Number of outputs outside the bound, and the worst |err| / (2^-24 ref_abs) seen."""
    got, ref, ref_abs = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, ref_abs))
    err = (got - ref).abs()
    bad = ~(err <= c * U32 * ref_abs + TINY)  # (NaN in got counts as outside)
    worst = float((err / (U32 * ref_abs + TINY)).nan_to_num(float("inf")).max()) if err.numel() else 0.0
    return int(bad.sum()), worst


def assert_bound(got, ref, ref_abs, c, what=""):
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    n, worst = violations(got, ref, ref_abs, c)
    assert n == 0, f"{what}: {n} outputs outside {c} * 2^-24 * sum|terms| (worst {worst:.1f})"


# ---------------------------------------------------------------- correlation2d
def corr2d(a, b, md, shift=0, drop=None):
    """out[b][k][y][x] = 1/C sum_c a[b][c][y][x] * b[b][c][y + dy_k][x + dx_k], zero outside; float64, differentiable.
    shift / drop plant faults for the self-checks: every tap read one column further right, or tap `drop` left out."""
    B, C, H, W = a.shape
    n = 2 * md + 1
    bp = torch.nn.functional.pad(b, (md, md + abs(shift), md, md))
    outs = []
    for k in range(n * n):
        dy, dx = k // n, k % n + shift
        t = (a * bp[:, :, dy:dy + H, dx:dx + W]).sum(1) / C
        outs.append(t * 0 if k == drop else t)
    return torch.stack(outs, 1)


def corr2d_backward(a, b, md, go, need=(True, True), **fault):
    """(grad_a, grad_b, |grad_a|-terms, |grad_b|-terms) of corr2d under grad_out go, by float64 autograd; the absolute
    forms are the same autograd over |a|, |b|, |go|."""
    def grads(a_, b_, go_):
        a_ = a_.detach().double().cpu().requires_grad_(need[0])
        b_ = b_.detach().double().cpu().requires_grad_(need[1])
        out = corr2d(a_, b_, md, **fault)
        out.backward(go_.detach().double().cpu().expand_as(out))
        return a_.grad, b_.grad
    ga, gb = grads(a, b, go)
    aa, ab = grads(a.abs(), b.abs(), go.abs())
    return ga, gb, aa, ab


# ---------------------------------------------------------------- 1x1 convolution + epilogue
def pointwise(x, w, scale=None, shift=None, residual=None, drop=None, shift_pos=0):
    """y[b][o][p] = scale[o] * sum_i w[o][i] x[b][i][p] + shift[o] (+ residual), x [B,Cin,P], w [Cout,Cin]; returns
    (y, sum of |terms|).  drop leaves input channel `drop` out, shift_pos reads position p + shift_pos (faults)."""
    x, w = x.double().cpu(), w.double().cpu().reshape(w.shape[0], -1)
    if drop is not None:
        w = w.clone()
        w[:, drop] = 0
    if shift_pos:
        x = torch.nn.functional.pad(x, (0, shift_pos))[:, :, shift_pos:]
    y, ya = torch.einsum("oi,bip->bop", w, x), torch.einsum("oi,bip->bop", w.abs(), x.abs())
    if scale is not None:
        s = scale.double().cpu().view(1, -1, 1)
        y, ya = y * s, ya * s.abs()
    if shift is not None:
        t = shift.double().cpu().view(1, -1, 1)
        y, ya = y + t, ya + t.abs()
    if residual is not None:
        r = residual.double().cpu().reshape(y.shape)
        y, ya = y + r, ya + r.abs()
    return y, ya
