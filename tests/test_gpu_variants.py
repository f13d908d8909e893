"""One case (or more) per kernel instantiation that no other test was written for, each shaped to sit on the host-side gate
that picks the instantiation (and where it matters one step either side), checked against a plain float64 restatement on
the CPU.  The ledger of which test launches which instantiation is tests/kernel_variants.py.

Linear operators (correlation2d and its backward, the 1x1 convolution) use the bound of tests/ref64.py:
|got - ref64| <= c * 2^-24 * sum|terms| + tiny, with c stated per operator; the CPU self-checks at the top of this file
show that one dropped term or one tap read a pixel off breaks it.  The normalising operators (LayerNorm, the attention
softmax) have no sum of terms to scale by; they keep a bound relative to the output scale, stated where used.  Every GPU
case runs a second time with torch.empty & co. handing out NaN / sentinel-filled memory (tests/poison.py) and must keep
its bits."""
import numpy as np
import pytest
import torch

from tests import ref64 as R
from tests.poison import check_unpoisoned

DEV = "cuda:0"
C_CORR = 8         # correlation2d backward: (2md+1)^2 fma in fp32 per element, 1/C folded into each tap
C_POINTWISE = 16   # 1x1 convolution: Cin fma per output in fp32 + scale / shift


def _seeded(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


# ---------------------------------------------------------------- CPU self-checks of the bound
def _fp32_corr_backward(a, b, md, go):
    """What a correct fp32 kernel could return: the float64 gradients rounded to fp32."""
    ga, gb, _, _ = R.corr2d_backward(a, b, md, go)
    return ga.float(), gb.float()


@pytest.mark.parametrize("md", [0, 1, 4, 5])
def test_bound_catches_planted_corr2d_faults(md):
    a, b = _seeded(1, 2, 9, 11, 13), _seeded(2, 2, 9, 11, 13)
    go = _seeded(3, 2, (2 * md + 1) ** 2, 11, 13)
    ga, gb, aa, ab = R.corr2d_backward(a, b, md, go)
    ga32, gb32 = _fp32_corr_backward(a, b, md, go)
    R.assert_bound(ga32, ga, aa, C_CORR, "fp32-rounded grad_in1")  # the bound admits a correct fp32 result
    R.assert_bound(gb32, gb, ab, C_CORR, "fp32-rounded grad_in2")
    for fault in ({"drop": (2 * md + 1) ** 2 // 2}, {"shift": 1}):
        fa, fb, _, _ = R.corr2d_backward(a, b, md, go, **fault)
        assert R.violations(fa.float(), ga, aa, C_CORR)[0] > 0, fault
        assert R.violations(fb.float(), gb, ab, C_CORR)[0] > 0, fault
    # and the forward
    out, out_abs = R.corr2d(a.double(), b.double(), md), R.corr2d(a.double().abs(), b.double().abs(), md)
    R.assert_bound(out.float(), out, out_abs, C_CORR)
    for fault in ({"drop": 0}, {"shift": 1}):
        assert R.violations(R.corr2d(a.double(), b.double(), md, **fault).float(), out, out_abs, C_CORR)[0] > 0, fault


def test_bound_catches_planted_pointwise_faults():
    x, w = _seeded(4, 2, 37, 135), _seeded(5, 50, 37) / 37 ** 0.5
    scale, shift, res = torch.rand(50) + 0.5, _seeded(6, 50), _seeded(7, 2, 50, 135)
    y, ya = R.pointwise(x, w, scale, shift, res)
    R.assert_bound(y.float(), y, ya, C_POINTWISE, "fp32-rounded 1x1 convolution")
    for fault in ({"drop": 36}, {"shift_pos": 1}):
        yf, _ = R.pointwise(x, w, scale, shift, res, **fault)
        assert R.violations(yf.float(), y, ya, C_POINTWISE)[0] > 0, fault


# ---------------------------------------------------------------- correlation2d backward: corr_backward_kernel<MD, *> and any md
def _corr_backward_case(B, C, H, W, md, seed, need=(True, True), dense_grad=True, batch_pad=0):
    from rpeflow_amd.csrc import wrapper as Wr
    a64, b64 = _seeded(seed, B, C, H, W), _seeded(seed + 1, B, C, H, W)
    K = (2 * md + 1) ** 2
    go = _seeded(seed + 2, B, K, H, W) if dense_grad else torch.ones(1, 1, 1, 1)

    def run():
        if batch_pad:  # B = 1 with a batch stride that is not C*H*W: a slice of a wider tensor, read where it lies
            a = torch.empty(B, C + batch_pad, H, W, device=DEV)[:, :C].copy_(a64)
        else:
            a = a64.to(DEV)
        a, b = a.requires_grad_(need[0]), b64.to(DEV).requires_grad_(need[1])
        out = Wr.correlation2d(a, b, md)
        if dense_grad:
            out.backward(go.to(DEV))
        else:
            out.sum().backward()  # grad_out: the expanded (stride 0) ones tensor
        return out.detach(), a.grad, b.grad

    out, g1, g2 = check_unpoisoned(run, f"correlation2d backward {(B, C, H, W, md)}")
    ref, ref_abs = R.corr2d(a64.double(), b64.double(), md), R.corr2d(a64.double().abs(), b64.double().abs(), md)
    R.assert_bound(out.cpu(), ref, ref_abs, C_CORR, f"forward {(B, C, H, W, md)}")
    ga, gb, aa, ab = R.corr2d_backward(a64, b64, md, go, need)
    if need[0]:
        R.assert_bound(g1.cpu(), ga, aa, C_CORR, f"grad_in1 {(B, C, H, W, md)}")
    else:
        assert g1 is None
    if need[1]:
        R.assert_bound(g2.cpu(), gb, ab, C_CORR, f"grad_in2 {(B, C, H, W, md)}")
    else:
        assert g2 is None


@pytest.mark.gpu
@pytest.mark.parametrize("md", range(8))
@pytest.mark.parametrize("C,H,W", [(1, 17, 15), (9, 16, 33), (33, 5, 47)])
def test_correlation2d_backward_every_md(md, C, H, W):
    """corr_backward_kernel<0..4, false/true> and the any-md path (md 5-7): tile edges (H, W % 16), the 8-channel staging
    tail (C % 8), B = 2."""
    _corr_backward_case(2, C, H, W, md, 7000 + 100 * md + C)


@pytest.mark.gpu
@pytest.mark.parametrize("md", [0, 4, 5])
@pytest.mark.parametrize("need", [(True, False), (False, True)])
def test_correlation2d_backward_one_input_strided_sum_grad(md, need):
    """Only one input needs a gradient, B = 1 read from a channel slice, and the stride-0 grad_out of out.sum()."""
    _corr_backward_case(1, 7, 19, 21, md, 7900 + md, need=need, dense_grad=False, batch_pad=3)


@pytest.mark.gpu
@pytest.mark.parametrize("md", [5, 7])
def test_correlation2d_autograd_wide_displacement(md):
    """correlation2d(a, b, 5 / 7) forward and backward through autograd (the backward refused md > 4 before)."""
    from rpeflow_amd.csrc import correlation2d
    a = _seeded(11, 1, 16, 24, 40).to(DEV).requires_grad_()
    b = _seeded(12, 1, 16, 24, 40).to(DEV).requires_grad_()
    correlation2d(a, b, md).sum().backward()
    assert a.grad is not None and b.grad is not None and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    _corr_backward_case(1, 16, 24, 40, md, 7950 + md)


# ---------------------------------------------------------------- 1x1 convolution: pointwise_conv_kernel<4 | 2, vec>
def _pointwise_case(B, Cin, Cout, P, seed, offset=0, inplace=False):
    from rpeflow_amd.utils import pointwise_conv
    x64 = _seeded(seed, B, Cin, P)
    w = _seeded(seed + 1, Cout, Cin, 1) / Cin ** 0.5
    scale, shift, res = torch.rand(Cout) + 0.5, _seeded(seed + 2, Cout) * 0.3, _seeded(seed + 3, B, Cout, P)

    def place(t):
        if not offset:
            return t.to(DEV)
        flat = torch.empty(t.numel() + offset, device=DEV)  # storage offset not a multiple of 4 floats
        return flat[offset:].view(t.shape).copy_(t)

    def run():
        x = place(x64)
        if inplace:
            r = place(res)
            y = pointwise_conv(x, w.to(DEV), None, residual=r, inplace=True)
            assert y.data_ptr() == r.data_ptr()
            return y
        return pointwise_conv(x, w.to(DEV), epilogue=(scale.to(DEV), shift.to(DEV), None))

    got = check_unpoisoned(run, f"pointwise_conv {(B, Cin, Cout, P, offset, inplace)}")[0]
    ref, ref_abs = R.pointwise(x64, w, None, None, res) if inplace else R.pointwise(x64, w, scale, shift)
    R.assert_bound(got.cpu(), ref, ref_abs, C_POINTWISE, f"pointwise_conv {(B, Cin, Cout, P, offset, inplace)}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,Cin,Cout,P,offset,inplace", [
    (2, 5, 241, 65536, 0, False),    # 16 output tiles (last one 1 channel wide), 8192 workgroups: <4, vec>
    (1, 7, 256, 131009, 0, False),   # P % 64 = 1, P % 4 = 1: <4, scalar>
    (2, 5, 241, 65536, 1, True),     # misaligned x and residual, accumulated in place: <4, scalar>
    (2, 5, 240, 65536, 0, False),    # one step under the tile gate (15 tiles): <2, vec>
    (1, 3, 250, 65536, 0, False),    # one step under the workgroup gate (4096 workgroups): <2, vec>
    (2, 5, 240, 65535, 0, False),    # under the tile gate with P % 4 = 3: <2, scalar>
])
def test_pointwise_conv_four_tile_gate(B, Cin, Cout, P, offset, inplace):
    _pointwise_case(B, Cin, Cout, P, 8100 + Cin + Cout, offset, inplace)


# ---------------------------------------------------------------- LayerNorm: channel_norm_kernel<CPT>
def _layernorm64(x, w, b, drop=None, shift=0):
    """LayerNorm over dim 1 in float64 (b None: the BiasFree form, no mean subtraction) and its rounding scale
    |w| (|x_hat| + 1) + |b|.  Faults: channel `drop` left out of the mean / variance, or every channel normalised with the
    statistics of the map shifted one pixel along W."""
    x = x.double()
    xs = x if drop is None else torch.cat([x[:, :drop], x[:, drop + 1:]], 1)
    if shift:
        xs = torch.roll(xs, shift, dims=-1)
    mu = xs.mean(1, keepdim=True) if b is not None else torch.zeros_like(x[:, :1])
    var = xs.var(1, keepdim=True, unbiased=False)
    xh = (x - mu) / torch.sqrt(var + 1e-5)
    wv = w.double().view(1, -1, 1, 1)
    bv = b.double().view(1, -1, 1, 1) if b is not None else torch.zeros_like(wv)
    return xh * wv + bv, wv.abs() * (xh.abs() + 1) + bv.abs()


@pytest.mark.parametrize("bias", [True, False])
def test_bound_catches_planted_layernorm_faults(bias):
    x, w = _seeded(21, 2, 64, 9, 15) + 0.5, torch.rand(64) + 0.5
    b = _seeded(22, 64) if bias else None
    ref, ref_abs = _layernorm64(x, w, b)
    R.assert_bound(ref.float(), ref, ref_abs, 32, "fp32-rounded LayerNorm")
    for fault in ({"drop": 63}, {"shift": 1}):
        assert R.violations(_layernorm64(x, w, b, **fault)[0].float(), ref, ref_abs, 32)[0] > 0, fault


@pytest.mark.gpu
@pytest.mark.parametrize("C", [33, 64, 97, 128, 193, 256])
@pytest.mark.parametrize("bias", [True, False])
def test_channel_layernorm_every_bucket(C, bias):
    """channel_norm_kernel<16> (C 33-64), <32> (97-128), <64> (193-256), both ends of each bucket, P % 64 != 0, both the
    WithBias and BiasFree forms.  Bound: 32 * 2^-24 * (|w| (|x_hat| + 1) + |b|) -- the rounding of a normalised value
    is relative to the normalised value itself plus the mean / variance reductions, which are O(1) after the scaling."""
    from rpeflow_amd.restormer_ops import channel_layernorm
    x64, w, b = _seeded(C, 2, C, 9, 15) + 0.5, torch.rand(C) + 0.5, _seeded(C + 1, C) if bias else None
    got = check_unpoisoned(lambda: channel_layernorm(x64.to(DEV), w.to(DEV), b.to(DEV) if bias else None),
                           f"channel_layernorm C={C}")[0].cpu()
    ref, ref_abs = _layernorm64(x64, w, b)
    R.assert_bound(got, ref, ref_abs, 32, f"channel_layernorm C={C} bias={bias}")


# ---------------------------------------------------------------- channel attention: attn_gram_kernel<T, R, vec>
ATTN_TOL = 1e-5  # of the largest |output|, about 170 * 2^-24: two normalisations, a softmax and two GEMMs in fp32


def _attn_matrix64(qkv, heads, temperature, w_out, eps=1e-12, drop=None, shift=0):
    """M[b] = W_out blockdiag_h(softmax(normalize(q_h) normalize(k_h)^T * t_h)) in float64 (restormer_arch.py:184-203 with
    v factored out).  Faults: position `drop` left out of the gram, or k read one position further along P."""
    qkv = qkv.double().cpu()
    B, C = qkv.shape[0], qkv.shape[1] // 3
    c = C // heads
    q, k = qkv[:, :C].reshape(B, heads, c, -1), qkv[:, C:2 * C].reshape(B, heads, c, -1)
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(eps)
    k = k / k.norm(dim=-1, keepdim=True).clamp_min(eps)
    if shift:
        k = torch.roll(k, shift, dims=-1)
    if drop is not None:
        q = q.clone()
        q[..., drop] = 0
    attn = ((q @ k.transpose(-2, -1)) * temperature.double().cpu().view(1, heads, 1, 1)).softmax(-1)
    m = torch.zeros(B, C, C, dtype=torch.float64)
    for h in range(heads):
        m[:, :, h * c:(h + 1) * c] = w_out.double().cpu().reshape(C, C)[:, h * c:(h + 1) * c] @ attn[:, h]
    return m


def test_bound_catches_planted_attention_faults():
    qkv, t, w = _seeded(31, 2, 3 * 64, 135), torch.rand(2) + 0.5, _seeded(32, 64, 64) / 8
    ref = _attn_matrix64(qkv, 2, t, w)
    tol = ATTN_TOL * float(ref.abs().max())
    assert float((ref.float().double() - ref).abs().max()) < tol  # a correctly rounded fp32 result passes
    for fault in ({"drop": 67}, {"shift": 1}):
        assert float((_attn_matrix64(qkv, 2, t, w, **fault).float().double() - ref).abs().max()) >= tol, fault


@pytest.mark.gpu
@pytest.mark.parametrize("B,heads,c,P", [(2, 2, 32, 135), (1, 1, 80, 16640)])
def test_attention_matrix_unpacked(B, heads, c, P):
    """channel_attention_matrix(packed=False) (attn_project_kernel<false>: M as a plain [B,C,C] matrix, the model only
    uses the packed form) against the float64 restatement."""
    from rpeflow_amd.restormer_ops import channel_attention_matrix
    C = heads * c
    qkv, t, w = _seeded(40 + c, B, 3 * C, P), torch.rand(heads) + 0.5, _seeded(41 + c, C, C) / C ** 0.5
    got = check_unpoisoned(lambda: channel_attention_matrix(qkv.to(DEV), heads, t.to(DEV), w.to(DEV), packed=False),
                           f"attention matrix {(B, heads, c, P)}")[0].cpu().double()
    ref = _attn_matrix64(qkv, heads, t, w)
    assert float((got - ref).abs().max()) < ATTN_TOL * max(float(ref.abs().max()), 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("c,spatial", [
    (64, (9, 15)), (80, (9, 15)),        # T = 4, 5 with one row group
    (64, (128, 130)), (64, (129, 129)),  # T = 4, R = 2 over P > 16384: vec (P % 4 = 0) and scalar
    (80, (128, 130)), (96, (129, 129)),  # T = 5, 6, R = 2: the last row group partial for T = 5
    (48, (128, 130)), (48, (129, 129)),  # T = 3, R = 3
    (64, (128, 128)),                    # P = 16384: one step under the R gate
    (80, (8, 16)),                       # T = 5, R = 1, vec
    (80, (129, 129)),                    # T = 5, R = 2, scalar: the last row group partial
    (96, (9, 15)),                       # T = 6, R = 1, scalar
    (32, (129, 129)),                    # T = 2, R = 2, scalar
])
def test_attention_gram_every_form(c, spatial):
    """Mutual attention with one head of c channels (T = ceil(c / 16) tile rows of the gram), B = 1, against the plain
    chain in float64.  Bound relative to the output scale: the softmax has no sum of |terms| to scale by; 1e-5 of the
    largest output (about 170 * 2^-24) for a chain of two normalisations, a softmax and two GEMMs."""
    from rpeflow_amd.model import _MutualAttention
    torch.manual_seed(c + spatial[0])
    m = _MutualAttention(c, 1, False, 2).eval()
    with torch.no_grad():
        m.temperature.uniform_(0.5, 3.0)
        x, y, r = (torch.randn(1, c, *spatial) for _ in range(3))
        ref = m.double()._forward_plain(x.double(), y.double())
        mg = m.float().to(DEV)
        got = check_unpoisoned(lambda: mg(x.to(DEV), y.to(DEV)), f"attention c={c} {spatial}")[0].cpu().double()
        got_r = check_unpoisoned(lambda: mg(x.to(DEV), y.to(DEV), residual=r.to(DEV)), "attention + residual")[0].cpu().double()
    tol = ATTN_TOL * max(float(ref.abs().max()), 1.0)
    assert float((got - ref).abs().max()) < tol, float((got - ref).abs().max())
    assert float((got_r - (r.double() + ref)).abs().max()) < tol


# ---------------------------------------------------------------- Correlation3D at C = 16: corr3d_cost / n2n <1>
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("N", [16, 130])
def test_correlation3d_sixteen_channels(N):
    """The cost and n2n kernels at C = 16 (one 16-channel tile) against the oracle, with the module tests' rule."""
    from oracle import oracle as O
    from rpeflow_amd import pwc3d_core as P3
    from tests import inputs as I
    from tests.test_oracle_golden import _shapes_corr3d
    r = I.rng(9116 + N)
    xyz1 = np.ascontiguousarray(I.ids_cloud(r, 2, N).transpose(0, 2, 1))
    xyz2 = (xyz1 + r.standard_normal(xyz1.shape, dtype=np.float32) * np.float32(0.2)).astype(np.float32)
    f1, f2 = r.standard_normal((2, 16, N), dtype=np.float32), r.standard_normal((2, 16, N), dtype=np.float32)
    params = I.fill_params(_shapes_corr3d(16), 4016 + N)
    m = P3.Correlation3D(16, 16, k=16)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    d = lambda a: torch.from_numpy(a).to(DEV)
    got = check_unpoisoned(lambda: m(d(xyz1), d(f1), d(xyz2), d(f2)), f"correlation3d C=16 N={N}")[0].cpu().numpy()
    ref = O.correlation3d(params, xyz1, f1, xyz2, f2, k=16)
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6 * float(np.abs(ref).max()) + 1e-6)


# ---------------------------------------------------------------- point searches: FPS, KNN, squared distance (index-exact)
@pytest.mark.gpu
@pytest.mark.parametrize("N,S", [(13000, 64), (16384, 5), (10000, 2048)])
def test_fps_wide_clouds(N, S):
    """fps_kernel_int<16, false> (N > 12794: the cloud no longer fits LDS) and fps_pruned2_kernel<16> (8192 < N <= 16384
    with S >= 2048), index-exact against the oracle."""
    from oracle import oracle as O
    from rpeflow_amd.csrc import furthest_point_sampling
    from tests import inputs as I
    pts = I.ids_cloud(I.rng(N + S), 1, N, 3)
    got = check_unpoisoned(lambda: furthest_point_sampling(torch.from_numpy(pts).to(DEV), S), f"fps {(N, S)}")[0].cpu().numpy()
    assert np.array_equal(got, O.furthest_point_sampling(pts, S))


@pytest.mark.gpu
@pytest.mark.parametrize("D,M,Q,k", [
    (1, 300, 8192, 1), (1, 300, 16384, 1), (2, 300, 16384, 1), (3, 300, 16384, 1),  # knn_nearest_kernel<D, 4 | 8>
    (1, 40, 5000, 1),                                                                # knn_select_kernel<1, 2, true>
    (1, 100, 16384, 3), (1, 200, 16384, 2), (2, 200, 16384, 2),                      # knn_select_kernel<1 | 2, 8, *>
])
def test_knn_queries_per_wave(D, M, Q, k):
    """The insertion / lane-minimum kernels at 2, 4 and 8 queries a wave (pick_qw: B * ceil(Q / qw) >= 2048), with and
    without the LDS row of topk's nth_element regime (M < 64 k), index- and distance-exact against the oracle."""
    from oracle import oracle as O
    from rpeflow_amd.csrc import wrapper as Wr
    from tests import inputs as I
    from tests.check import assert_bits_equal
    r = I.rng(D * 1000 + M + Q + k)
    inp, qry = I.ids_cloud(r, 1, M, D), I.ids_cloud(r, 1, Q, D)
    idx, dist = check_unpoisoned(lambda: Wr.k_nearest_neighbor_with_distances(torch.from_numpy(inp).to(DEV), torch.from_numpy(qry).to(DEV),
                                                                              k, algo="insert"), f"knn {(D, M, Q, k)}")
    oi, od = O.k_nearest_neighbor(inp, qry, k, return_dists=True)
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert_bits_equal(dist.cpu().numpy(), od, str((D, M, Q, k)))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 2, 3])
def test_squared_distance_every_dimension(D):
    """sqdist_kernel<D> against the float64 restatement |a|^2 + |b|^2 - 2 a.b (the reference's matmul form), bound
    8 * 2^-24 * (|a|^2 + |b|^2 + 2 |a||b|)."""
    from rpeflow_amd.csrc import squared_distance
    a, b = _seeded(50 + D, 2, 37, D) * 3, _seeded(60 + D, 2, 301, D) * 3
    got = check_unpoisoned(lambda: squared_distance(a.to(DEV), b.to(DEV)), f"sqdist D={D}")[0].cpu()
    a64, b64 = a.double(), b.double()
    n1, n2 = (a64 ** 2).sum(-1)[:, :, None], (b64 ** 2).sum(-1)[:, None, :]
    ref = n1 + n2 - 2 * a64 @ b64.transpose(1, 2)
    ref_abs = n1 + n2 + 2 * a64.abs() @ b64.abs().transpose(1, 2)
    R.assert_bound(got, ref, ref_abs, 8, f"squared_distance D={D}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 8])
def test_knn_interpolation_wide_k(k):
    """knn_interp_kernel<8> (4 <= k <= 8) against the oracle, with the fuzz test's rule."""
    from oracle import oracle as O
    from rpeflow_amd import utils as U
    from tests import inputs as I
    r = I.rng(300 + k)
    a = np.ascontiguousarray(I.ids_cloud(r, 2, 500).transpose(0, 2, 1))
    q = np.ascontiguousarray(I.ids_cloud(r, 2, 700).transpose(0, 2, 1))
    feat = r.standard_normal((2, 19, 500), dtype=np.float32)
    d = lambda t: torch.from_numpy(t).to(DEV)
    got = check_unpoisoned(lambda: U.knn_interpolation(d(a), d(feat), d(q), k=k), f"knn_interpolation k={k}")[0].cpu().numpy()
    ref = O.knn_interpolation(a, feat, q, k=k)
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.gpu
@torch.no_grad()
def test_pointconv_widest_tile():
    """pointconv_fused_kernel<2, 2, 4, 2, 1> (Cout > 64 and B Q ceil(Cout / 128) >= 64 x 512): 384 outputs over 11000
    points, against the oracle with the module tests' rule."""
    from oracle import oracle as O
    from rpeflow_amd import pointconv as PC
    from tests import inputs as I
    from tests.test_oracle_golden import _shapes_pointconv
    r = I.rng(7384)
    xyz = np.ascontiguousarray(I.ids_cloud(r, 1, 11000).transpose(0, 2, 1))
    feat = r.standard_normal((1, 8, 11000), dtype=np.float32)
    params = I.fill_params(_shapes_pointconv(8, 384, None), 7384)
    m = PC.PointConvNoSampling(8, 384, norm=None)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    d = lambda t: torch.from_numpy(t).to(DEV)
    got = check_unpoisoned(lambda: m(d(xyz), d(feat)), "pointconv 8 -> 384")[0].cpu().numpy()
    ref = O.pointconv(params, xyz, feat, k=16)
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6 * float(np.abs(ref).max()) + 1e-6)
