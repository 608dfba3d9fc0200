"""CPU self-checks of the numeric references in pyref.py (the oracles of
test_gpu_feature_edges.py and test_gpu_fm_edges.py), so that those tests do
not rest on an unchecked reference or on torch alone."""
import numpy as np
import torch

import pyref


def _torch_e4m3(x32: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(
        torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_e4m3_table_matches_torch_decode():
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    np.testing.assert_array_equal(np.isnan(pyref.E4M3), np.isnan(want))
    fin = ~np.isnan(want)
    np.testing.assert_array_equal(pyref.E4M3[fin], want[fin])
    np.testing.assert_array_equal(np.signbit(pyref.E4M3[fin]), np.signbit(want[fin]))
    assert len(pyref.E4M3_FINITE) == 254 and fin.sum() == 254
    assert np.nanmax(pyref.E4M3) == 448.0 == pyref.E4M3_MAX
    assert pyref.E4M3[1] == 2.0 ** -9  # smallest subnormal


def test_torch_e4m3_cast_is_nearest_even_on_the_edge_values():
    """torch's CPU float32 -> float8_e4m3fn cast (the oracle of the fp8 tests)
    equals a nearest-even search over the 254 decoded codes at every edge
    value, and has the properties the tests rely on."""
    vals = pyref.fp8_edge_values()
    got = _torch_e4m3(vals)
    np.testing.assert_array_equal(got, pyref.e4m3_nearest_even(vals))
    # every finite code is its own image; every midpoint goes to the even code
    mag = pyref.E4M3[:0x7F].astype(np.float32)
    np.testing.assert_array_equal(_torch_e4m3(mag), np.arange(0x7F, dtype=np.uint8))
    np.testing.assert_array_equal(_torch_e4m3(-mag), np.arange(0x7F, dtype=np.uint8) | 0x80)
    mids = ((mag[:-1].astype(np.float64) + mag[1:]) / 2).astype(np.float32)
    lo = np.arange(0x7E)
    np.testing.assert_array_equal(_torch_e4m3(mids), np.where(lo % 2 == 0, lo, lo + 1))
    one = lambda v: int(_torch_e4m3(np.array([v], np.float32))[0])  # noqa: E731
    assert one(2.0 ** -10) == 0x00
    assert one(np.nextafter(np.float32(2.0 ** -10), np.float32(1))) == 0x01
    assert one(-0.0) == 0x80
    assert one(464.0) == 0x7E and one(-464.0) == 0xFE
    # past 464 torch gives NaN (the hardware's answer is pinned by the GPU test)
    assert one(np.nextafter(np.float32(464), np.float32(1e9))) & 0x7F == 0x7F
    # a random sweep of the whole finite range
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-12, 9, 200000))).astype(np.float32)
    x = x[np.abs(x) <= 464]
    np.testing.assert_array_equal(_torch_e4m3(x), pyref.e4m3_nearest_even(x))


def test_edge_value_set_is_complete():
    vals = pyref.fp8_edge_values()
    have = set(vals.view(np.uint32).tolist())
    mag = pyref.E4M3[:0x7F].astype(np.float32)
    for s in (1.0, -1.0):
        for v in mag:
            assert np.float32(s * v).view(np.uint32) in have
        for a, b in zip(mag[:-1], mag[1:]):
            m = np.float32(s * (float(a) + float(b)) / 2)
            for t in (m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf))):
                assert np.float32(t).view(np.uint32) in have
    assert np.float32(-0.0).view(np.uint32) in have and np.float32(0.0).view(np.uint32) in have
    oor = pyref.fp8_out_of_range_values()
    assert np.all((np.abs(oor) > 464) | np.isnan(oor))


def test_bf16_round_matches_torch():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(100000) * np.exp2(rng.integers(-30, 30, 100000))).astype(np.float32)
    # exact ties between two bf16 values, both parities
    ties = (np.arange(1, 2000, dtype=np.uint32) << 16 | 0x8000).view(np.float32)
    x = np.concatenate([x, ties, -ties, np.zeros(1, np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(pyref.bf16_round(x), want)


def test_hash_reference_is_murmur_fmix64():
    # the published fmix64 test vector: fmix64(1) with no seed
    assert int(pyref.ref_hash(np.array([1], np.uint64), 0)[0]) == 0xB456BCFC34C2CB2C & 0xFFFFFFFF
    # 64-bit keys are not truncated: keys equal below bit 32 hash apart
    a, b = pyref.ref_hash(np.array([5, 5 + (1 << 33)], np.uint64), 3)
    assert a != b


def test_fm_gradient_formula_matches_autograd():
    """F3 / F4's formula (dw = s Z_0, dV = s Z_{1+f} - V s^2 t with Z = G^T x,
    G = [g, g xv], t = (x^2)^T g) is the gradient of HashedFM.reference: fp64
    autograd of that function, and fp32 autograd within its own rounding."""
    from dmlc_core_amd.models import HashedFM
    rng = np.random.default_rng(2)
    rows, dim, s = 23, 40, 0.5
    codes = rng.choice(pyref.E4M3_FINITE, size=(rows, dim))
    xq = pyref.E4M3[codes] / 16  # the quantised batch
    w = rng.standard_normal((dim, 1)) * 0.1
    v = rng.standard_normal((dim, 16)) * 0.1
    r = rng.standard_normal(rows)
    x = xq * s  # the dequantised features the model sees
    for dt, tol in ((torch.float64, 1e-11), (torch.float32, 2e-4)):
        wt = torch.tensor(w, dtype=dt, requires_grad=True)
        vt = torch.tensor(v, dtype=dt, requires_grad=True)
        bt = torch.zeros(1, dtype=dt, requires_grad=True)
        y = HashedFM.reference(torch.tensor(x, dtype=dt), wt, vt, bt)
        (y * torch.tensor(r, dtype=dt)).sum().backward()
        xv = x @ v  # = s xq V, what F1 writes
        gm = np.concatenate([r[:, None], r[:, None] * xv], axis=1)
        z = np.concatenate([gm.T @ xq, (r[None, :] @ (xq * xq))], axis=0)
        dw, dv, _, _ = pyref.fm_grads_ref(z[None], v, s)
        scale = max(np.abs(dv).max(), np.abs(dw).max())
        assert np.abs(wt.grad.numpy()[:, 0] - dw).max() <= tol * scale
        assert np.abs(vt.grad.numpy() - dv).max() <= tol * scale


def test_fm_forward_reference_matches_model_reference():
    from dmlc_core_amd.models import HashedFM
    rng = np.random.default_rng(3)
    rows, dim, s = 9, 128, 0.25
    codes = rng.choice(pyref.E4M3_FINITE, size=(rows, dim)).astype(np.uint8)
    wt = pyref.bf16_round((rng.standard_normal((17, dim)) * 0.05).astype(np.float32))
    v = wt[1:].T.astype(np.float64)
    q = (v * v).sum(1)
    y, xv, y_tol, xv_tol = pyref.fm_forward_ref(codes, wt, q, 0.3, s)
    x = torch.tensor(pyref.E4M3[codes] * s)
    want = HashedFM.reference(x, torch.tensor(wt[0].astype(np.float64))[:, None], torch.tensor(v),
                              torch.tensor([0.3], dtype=torch.float64)).numpy()
    np.testing.assert_allclose(y, want, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(xv, (x @ torch.tensor(v)).numpy(), rtol=1e-12, atol=1e-12)
    assert np.all(y_tol > 0) and np.all(y_tol < 1e-2 * (np.abs(want) + 1) * dim)
    assert np.all(xv_tol >= 0)


def test_csr_references():
    off = np.array([2, 2, 5, 6])
    idx = np.array([9, 9, 0, 1, 0, 2, 9])
    val = np.array([9, 9, 1.5, 2.0, -1.0, 4.0, 9], np.float32)
    w = np.array([1.0, 10.0, 100.0])
    y, tol = pyref.csr_dot_ref(off, idx, val, w, 0.5)
    np.testing.assert_array_equal(y, [0.5, 1.5 + 20 - 1 + 0.5, 400.5])
    assert tol[0] == 4 * pyref.U24 * 0.5
    g, gtol = pyref.csr_dot_t_ref(off, idx, val, np.array([7.0, 2.0, 3.0]), 3)
    np.testing.assert_array_equal(g, [3 - 2, 4.0, 12.0])
    y1, _ = pyref.csr_dot_ref(off, idx, None, w)
    np.testing.assert_array_equal(y1, [0, 12, 100])
