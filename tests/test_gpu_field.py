"""GPU parity of the SuGaR density field (forward + backward), the level-set surface sampler and the row-gather backward against
the PyTorch restatement of the reference's tensor code (oracle/sugar_field_torch.py), run in float64 on the float32-rounded inputs.

Bars are per element: |HIP - ref64| <= c * 2^-24 * m, where m is the element's condition magnitude from the float64 restatement
(the sum of |term| of every sum, (1 + |argument|) |value| for every exponential; oracle/sugar_field_torch.py).  One dropped or
doubled term of relative size 1e-4 of m exceeds every c below (1e-4 * 2^24 = 1678).  Each c is about twice the largest ratio
measured on an MI355X over every case (in brackets below).
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import sugar_field_torch as ref
from oracle.torch_cpu_rasterizer import quat_to_rotmat

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# c per output and the kernels that write it; in brackets the largest measured max |HIP - ref64| / (2^-24 m) over every case
C_OPAC = 8        # k_density_fwd16 / k_density_fwd, neighbor_opacities  [6.44]
C_DENS = 8        # k_density_fwd16 (DPP row sum) / k_density_fwd (sequential), densities  [3.77]
C_DX = 8          # k_density_dx16 / k_density_dx / k_density_bwd, dL/dx  [3.03]
C_GAUSS = 16      # k_density_bwd_gather (or k_density_bwd's float atomics): dL/dcentres, dL/dB, dL/dstrengths  [5.15]
C_HOT = 16        # the same for the Gaussian in every list (~N pairs: sixteen strided sums of N / 16 terms)  [0.39]
C_ROWS = 8        # k_rows_gather (sgr_scatter_add_rows)  [2.19]
C_ROWS_HOT = 64   # a row that a third of 17.5M entries hit


def _rot(P, g):
    return quat_to_rotmat(torch.nn.functional.normalize(torch.randn(P, 4, generator=g, dtype=torch.float64), dim=-1))


def _field_case(P, N, K, seed, edges=True):
    """A scene of P Gaussians (spacing ~0.05, scales ~0.03) and N samples near them, each with the K nearest Gaussians of a random
    Gaussian as its neighbours (SuGaR's knn_idx[gaussian_idx]).  With `edges`: one large Gaussian (1) in every list (K >= 8);
    every Gaussian i with i % 97 == 2 referenced by no sample; a neighbour twice in rows n % 101 == 3; samples at a centre
    (q = 0) in rows n % 211 == 5; samples 1e5 away (q > 1e8) in rows n % 307 == 7; strength 0 for i % 53 == 11.
    Everything is rounded to float32 and returned in float64 on the CPU."""
    from scipy.spatial import cKDTree
    g = torch.Generator().manual_seed(seed)
    side = 0.05 * P ** (1. / 3.)
    ce = torch.rand(P, 3, generator=g, dtype=torch.float64) * side
    scales = 0.03 * torch.exp(0.4 * torch.randn(P, 3, generator=g, dtype=torch.float64))
    R = _rot(P, g)
    st = torch.rand(P, 1, generator=g, dtype=torch.float64)
    gi = torch.randint(0, P, (N,), generator=g)
    x = ce[gi] + 0.03 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    if N:
        _, idx = cKDTree(ce.numpy()).query(ce[gi].numpy(), k=K, workers=16)
        nb = torch.as_tensor(np.asarray(idx).reshape(N, K), dtype=torch.int64)
    else:
        nb = torch.zeros(0, K, dtype=torch.int64)
    meta = dict(hot=None, dead=torch.zeros(P, dtype=torch.bool), far=torch.zeros(N, dtype=torch.bool))
    if edges:
        ar = torch.arange(P)
        st[ar % 53 == 11] = 0.
        dead = ar % 97 == 2
        nb = torch.where(nb % 97 == 2, nb - 1, nb)
        rows = torch.arange(N)
        if K >= 2:
            nb[rows % 101 == 3, 1] = nb[rows % 101 == 3, 0]
        if K >= 8:
            meta["hot"] = 1
            nb[:, K - 1] = 1
            scales[1] = side
            st[1] = 0.5
        at = rows % 211 == 5
        x[at] = ce[nb[at, 0]]
        far = rows % 307 == 7
        x[far] += 1e5
        meta.update(dead=dead, far=far)
        assert not bool(torch.isin(torch.nonzero(dead)[:, 0], nb.reshape(-1)).any())
    B = R * (1.0 / scales)[:, None]
    r32 = lambda t: t.float().double()
    return r32(x), nb, r32(ce), r32(B), r32(st), meta


def _ratio(got, want, mag):
    """max over the elements of |got - want| / (2^-24 mag); an element with mag == 0 must be exact (else inf)"""
    err = (got.detach().double().to(want.device) - want).abs()
    r = err / (U * mag)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


def _rel(a, b):
    a = a.detach().double().to(b.device)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _run_density(x, nb, ce, B, st, factor, go, gd):
    from sugar_amd.field import density_field
    xd = x.float().to(DEV).requires_grad_(True); cd = ce.float().to(DEV).requires_grad_(True)
    Bd = B.float().to(DEV).requires_grad_(True); sd = st.float().to(DEV).requires_grad_(True)
    o, d = density_field(xd, nb.to(DEV), cd, Bd, sd, factor)
    ((o * go.float().to(DEV)).sum() + (d * gd.float().to(DEV)).sum()).backward()
    return dict(opacities=o.detach(), densities=d.detach(), dx=xd.grad, dcenters=cd.grad, dB=Bd.grad, dstrengths=sd.grad[:, 0])


def _grads_in(N, K, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return (torch.randn(N, K, generator=g, dtype=torch.float64).float().double(),
            torch.randn(N, generator=g, dtype=torch.float64).float().double())


def _check_density(tag, got, x, nb, ce, B, st, meta, factor, go, gd):
    """every output element against the float64 restatement; returns the measured ratios (also printed)"""
    r = ref.density_field_chunked(x.to(DEV), nb.to(DEV), ce.to(DEV), B.to(DEV), st.to(DEV), factor, go.to(DEV), gd.to(DEV))
    bars = dict(opacities=C_OPAC, densities=C_DENS, dx=C_DX, dcenters=C_GAUSS, dB=C_GAUSS, dstrengths=C_GAUSS)
    hot = meta["hot"]
    keep = torch.ones(ce.shape[0], dtype=torch.bool, device=DEV)
    if hot is not None:
        keep[hot] = False
    ratios = {}
    for k, c in bars.items():
        a, w, m = got[k].reshape(r[k].shape), r[k], r[k + "_mag"]
        if k in ("dcenters", "dB", "dstrengths"):
            ratios[k] = _ratio(a[keep], w[keep], m[keep])
            if hot is not None:
                ratios[k + "_hot"] = _ratio(a[hot], w[hot], m[hot])
        else:
            ratios[k] = _ratio(a, w, m)
    print("RATIO", tag, " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        c = C_HOT if k.endswith("_hot") else bars[k]
        assert v <= c, (tag, k, v, c)
    # the edges, exactly
    dead = meta["dead"].to(DEV)
    if bool(dead.any()):
        for k in ("dcenters", "dB", "dstrengths"):
            assert float(got[k][dead].abs().max()) == 0.0, (tag, k)
    far = meta["far"].to(DEV)
    if bool(far.any()):
        assert float(got["opacities"][far].abs().max()) == 0.0 and float(got["dx"][far].abs().max()) == 0.0
    # the norm-wise bars these replace stay
    assert _rel(got["opacities"], r["opacities"]) < 1e-5 and _rel(got["densities"], r["densities"]) < 1e-5
    for k in ("dx", "dcenters", "dB", "dstrengths"):
        assert _rel(got[k].reshape(r[k].shape), r[k]) < 1e-4, k
    return r


DENSITY_CASES = {
    # id: (P, N, K, factor, use_gather, seed)
    "k16": (4000, 20000, 16, 1.3, True, 5),
    "k1": (3000, 9999, 1, 0.2, True, 6),
    "k8": (5000, 30001, 8, 1.0, True, 7),
    "k17": (4000, 12345, 17, 1.3, True, 8),
    "k32": (6000, 7777, 32, 1.0, True, 9),
    "k16_atomics": (4000, 20003, 16, 1.3, False, 10),
    "k8_atomics": (3000, 10001, 8, 0.2, False, 11),
    "trainer_1M": (1_000_000, 1_000_000, 16, 1.0, True, 12),
    "trainer_1.1M": (200_000, 1_100_000, 16, 1.0, True, 13),
}


@pytest.mark.parametrize("case", list(DENSITY_CASES))
def test_density_field_forward_backward(case):
    """Every dispatch of the density field against the float64 restatement, per element.  K == 16 runs k_density_fwd16 and
    k_density_dx16, any other K k_density_fwd and k_density_dx; the per-Gaussian gradients come from k_density_bwd_gather
    after the radix grouping (2 passes for P < 65536, 3 for the trainer cases; 16M+ pairs run k_fscan_top with per = 2), or
    with _DensityField.use_gather = False from the float atomics of k_density_bwd.  Every case but K = 1 has a Gaussian in every
    list; all have unreferenced Gaussians (rows exactly 0), repeated neighbours, q = 0, q > 1e8 (exactly 0) and strength 0."""
    from sugar_amd.field import _DensityField
    P, N, K, factor, gather, seed = DENSITY_CASES[case]
    x, nb, ce, B, st, meta = _field_case(P, N, K, seed)
    go, gd = _grads_in(N, K, seed)
    old = _DensityField.use_gather
    _DensityField.use_gather = gather
    try:
        got = _run_density(x, nb, ce, B, st, factor, go, gd)
        _check_density(case, got, x, nb, ce, B, st, meta, factor, go, gd)
        if case == "trainer_1.1M":   # the radix grouping orders every sum: the backward is reproducible bit for bit
            again = _run_density(x, nb, ce, B, st, factor, go, gd)
            for k in ("dx", "dcenters", "dB", "dstrengths"):
                assert torch.equal(again[k], got[k]), k
    finally:
        _DensityField.use_gather = old
    assert got["dB"].shape == (P, 3, 3) and got["dstrengths"].shape == (P,)


@pytest.mark.parametrize("gather", [True, False])
def test_density_field_with_no_samples(gather):
    """N = 0: empty outputs, and every gradient row is written, exactly 0 (the gather path groups nothing through the atomics scan)"""
    from sugar_amd.field import _DensityField
    x, nb, ce, B, st, _ = _field_case(5000, 0, 16, 3, edges=False)
    old = _DensityField.use_gather
    _DensityField.use_gather = gather
    try:
        got = _run_density(x, nb, ce, B, st, 1.0, torch.zeros(0, 16, dtype=torch.float64), torch.zeros(0, dtype=torch.float64))
    finally:
        _DensityField.use_gather = old
    assert got["opacities"].shape == (0, 16) and got["densities"].shape == (0,) and got["dx"].shape == (0, 3)
    for k in ("dcenters", "dB", "dstrengths"):
        assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) == 0.0, k


@pytest.mark.parametrize("K", [16, 8])
def test_density_field_c_abi_optional_pointers(K):
    """`packed = NULL` gives the packed call's bits; dL_dopacities = NULL and dL_ddensity = NULL each give the bits of the call with
    that gradient passed as zeros (sgr_density_field_forward, sgr_density_field_backward_gather)"""
    from sugar_amd import _lib
    from sugar_amd.field import _pack, _p, _stream
    lib = _lib.load()
    x, nb, ce, B, st, _ = _field_case(4000, 10007, K, 21, edges=False)
    go, gd = _grads_in(10007, K, 21)
    N, P = x.shape[0], ce.shape[0]
    xs, nbd, cd, Bd, sd = x.float().to(DEV), nb.to(DEV), ce.float().to(DEV), B.float().reshape(P, 9).to(DEV), st.float().reshape(P).to(DEV)
    god, gdd = go.float().to(DEV), gd.float().to(DEV)
    packed = _pack(lib, cd, Bd, sd)

    def fwd(pk):
        o, d = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
        with torch.cuda.device(DEV):
            assert lib.sgr_density_field_forward(N, K, _p(xs), _p(nbd), _p(cd), _p(Bd), _p(sd), 1.3, _p(o), _p(d), _p(pk), _stream(DEV)) == 0
        return o, d

    def bwd(g_o, g_d):
        out = [torch.full((N, 3), 7.0, device=DEV), torch.full((P, 3), 7.0, device=DEV), torch.full((P, 9), 7.0, device=DEV),
               torch.full((P,), 7.0, device=DEV)]
        scratch = torch.empty(lib.sgr_density_field_backward_scratch_bytes(N, K, P), dtype=torch.uint8, device=DEV)
        with torch.cuda.device(DEV):
            rc = lib.sgr_density_field_backward_gather(N, K, P, _p(xs), _p(nbd), _p(cd), _p(Bd), _p(sd), 1.3, _p(g_o), _p(g_d),
                                                       *[_p(t) for t in out], _p(scratch), _p(packed), _stream(DEV))
        assert rc == 0
        return out

    a, b = fwd(packed), fwd(None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for got, want in ((bwd(None, gdd), bwd(torch.zeros_like(god), gdd)), (bwd(god, None), bwd(god, torch.zeros_like(gdd)))):
        for u, v in zip(got, want):
            assert torch.equal(u, v)
    full = bwd(god, gdd)
    r = ref.density_field_chunked(x.to(DEV), nbd, ce.to(DEV), B.to(DEV), st.to(DEV), 1.3, go.to(DEV), gd.to(DEV))
    assert _ratio(full[0], r["dx"], r["dx_mag"]) <= C_DX and _ratio(full[3], r["dstrengths"], r["dstrengths_mag"]) <= C_GAUSS
    assert _rel(a[1], r["densities"]) < 1e-5


@pytest.mark.parametrize("K", [16, 8])
@pytest.mark.parametrize("N", [1, 257])
def test_sdf_field_carries_the_density_fields_bits(N, K):
    """sdf_field and density_field run the two instances of one kernel family (csrc/field.hip, template <bool SDF>).  Asserted, bit
    for bit: the neighbour opacities and the density of the two (the contract the SDF field documents), and -- with no gradient for
    beta and sdf -- dcenters and dB of the backward; dmin_scaling is exactly 0 and so is every gradient row of an unreferenced
    Gaussian.  P = 300 with 60 Gaussians that no sample references, a neighbour twice in row 0, factor 1.3, threshold 1.

    While the SDF forward kept its pair arithmetic under the range check's branch the forward equalities did NOT hold (MI355X; also
    with the separate k_sdf_* kernels before the family): the compiler paired the products of w = B^T d and |w|^2 into packed FP32
    instructions there (one product rounded on its own) and left the density kernels scalar FMA chains; opacities differed by up to
    8.94e-08, densities by 1.19e-07 at these shapes.  The SDF forward now runs the arithmetic for every lane and discards the
    out-of-range ones.  Backward outputs that were not bit-equal before the family either, and are printed, not asserted: dx
    (N = 257, K = 16: max |diff| 1.91e-06; equal in the other three cases) and dstrengths (N = 257, K = 16: 1.49e-08; equal in the
    other three)."""
    from sugar_amd.sdf_regulariser import sdf_field
    P, used, factor = 300, 240, 1.3
    g = torch.Generator().manual_seed(1000 * N + K)
    ce = torch.rand(P, 3, generator=g, dtype=torch.float64) * 0.3
    B = _rot(P, g) * (1.0 / (0.03 * torch.exp(0.4 * torch.randn(P, 3, generator=g, dtype=torch.float64))))[:, None]
    st = torch.rand(P, 1, generator=g, dtype=torch.float64)
    ms = 0.01 + 0.02 * torch.rand(P, generator=g)
    nb = torch.randint(0, used, (N, K), generator=g)
    nb[0, 1] = nb[0, 0]
    x = ce[nb[:, 0]] + 0.03 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    go, gd = _grads_in(N, K, 77)
    want = _run_density(x, nb, ce, B, st, factor, go, gd)

    leaves = [t.float().to(DEV).requires_grad_(True) for t in (x, ce, B, st, ms)]
    o, d, beta, sdf = sdf_field(leaves[0], nb.to(DEV), *leaves[1:], factor, 1.0, 1e-16)
    ((o * go.float().to(DEV)).sum() + (d * gd.float().to(DEV)).sum()).backward()
    got = dict(opacities=o.detach(), densities=d.detach(), dx=leaves[0].grad, dcenters=leaves[1].grad, dB=leaves[2].grad,
               dstrengths=leaves[3].grad[:, 0])
    assert float(want["opacities"].abs().max()) > 0 and float(want["dB"].abs().max()) > 0
    for k, w in want.items():
        print("EQUAL", N, K, k, bool(torch.equal(got[k], w)), f"max |diff| = {float((got[k] - w).abs().max()):.3g}")
    assert float(leaves[4].grad.abs().max()) == 0.0
    for k in ("dcenters", "dB", "dstrengths"):
        assert float(got[k][used:].abs().max()) == 0.0, k
    for k in ("dcenters", "dB", "opacities", "densities"):
        assert torch.equal(got[k], want[k]), k


ATOMICS_CASE = dict(P=2_500_000, N=200_003, K=16, factor=1.3, seed=31)   # P > 2^21: the P-scan's k_fscan_top runs with per = 2
ATOMICS_ROWS = dict(M=3_000_001, W=3, P=2_500_000, seed=32)


def _rows_case(M, W, P, seed, hot=False):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, P, (M,), generator=g)
    if hot:
        idx[1::3] = 5                         # a third of all entries in one row
    idx[idx == 3] = 4                         # a row nobody gathers
    idx[::7] -= P                             # Python-style negative indices
    src = torch.randn(M, W, generator=g)
    return idx, src


def _rows_ref(idx, src, P):
    """float64 index_add_ and the per-row sum of |term|"""
    ix = torch.where(idx < 0, idx + P, idx).to(DEV)
    s = src.double().to(DEV)
    out = ref.add_rows(torch.zeros(P, s.shape[1], dtype=torch.float64, device=DEV), ix, s)
    mag = ref.add_rows(torch.zeros_like(out), ix, s.abs())
    return out, mag


def _atomics_child(path):
    """run in a fresh process with SGR_GROUP_ATOMICS=1 (read once per process): the density backward and the row scatter grouped by
    returning integer atomics (k_density_bwd_rank, k_density_bwd_fill, k_rows_rank, k_rows_fill)"""
    from sugar_amd.row_gather import row_gather
    c = ATOMICS_CASE
    x, nb, ce, B, st, _ = _field_case(c["P"], c["N"], c["K"], c["seed"])
    go, gd = _grads_in(c["N"], c["K"], c["seed"])
    got = _run_density(x, nb, ce, B, st, c["factor"], go, gd)
    rc = ATOMICS_ROWS
    idx, src = _rows_case(rc["M"], rc["W"], rc["P"], rc["seed"])
    a = torch.zeros(rc["P"], rc["W"], device=DEV, requires_grad=True)
    row_gather(a, idx.to(DEV)).backward(src.to(DEV))
    got["rows"] = a.grad
    torch.save({k: v.cpu() for k, v in got.items()}, path)


def test_group_atomics_mode_in_a_fresh_process():
    """SGR_GROUP_ATOMICS=1 (the round-4 grouping, kept for same-box comparison) at P = 2.5M, per element like the default path"""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.pt")
        code = (f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_field import _atomics_child; "
                f"_atomics_child({path!r})")
        env = dict(os.environ, SGR_GROUP_ATOMICS="1")
        try:
            p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=600, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.exit("the SGR_GROUP_ATOMICS=1 child timed out: no further GPU test starts", returncode=3)
        if p.returncode in (134, 139, -6, -11):
            pytest.exit(f"the SGR_GROUP_ATOMICS=1 child died ({p.returncode}): no further GPU test starts\n{p.stderr[-4000:]}",
                        returncode=3)
        assert p.returncode == 0, p.stderr[-4000:]
        got = {k: v.to(DEV) for k, v in torch.load(path).items()}
    c = ATOMICS_CASE
    x, nb, ce, B, st, meta = _field_case(c["P"], c["N"], c["K"], c["seed"])
    go, gd = _grads_in(c["N"], c["K"], c["seed"])
    _check_density("group_atomics", got, x, nb, ce, B, st, meta, c["factor"], go, gd)
    rc = ATOMICS_ROWS
    idx, src = _rows_case(rc["M"], rc["W"], rc["P"], rc["seed"])
    want, mag = _rows_ref(idx, src, rc["P"])
    r = _ratio(got["rows"], want, mag)
    print("RATIO group_atomics rows", f"{r:.3g}")
    assert r <= C_ROWS and float(got["rows"][3].abs().max()) == 0.0


C_PT = 16         # k_level_set: the intersection point beyond what the densities' bars allow (the float32 t grid, the lerp, p + t dir)
C_NRM = 32        # k_level_set: the density gradient at the point, relative to its condition magnitude
LEVELS = {1: (0.3,), 3: (0.1, 0.3, 0.5), 8: (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.8)}
LS_CASES = {
    # id: (P, N, K, n_points_in_range, range_size, n_levels, density_factor, seed)
    "r21": (6000, 30000, 16, 21, 3.0, 3, 1.0, 9),
    "r2": (4000, 20001, 8, 2, 3.0, 1, 1.0, 40),
    "r3": (4000, 20001, 16, 3, 0.25, 3, 1.7, 41),
    "r20": (4000, 20001, 1, 20, 3.0, 8, 1.0, 42),
    "r22": (4000, 20001, 32, 22, 3.0, 3, 1.7, 43),
    "r31": (4000, 20001, 16, 31, 0.25, 8, 1.0, 44),
    "r32": (4000, 20001, 8, 32, 3.0, 1, 1.7, 45),
    "r21_2M": (200_000, 2_000_003, 16, 21, 3.0, 3, 1.0, 46),
}
N_EDGE = 4   # pixels per edge kind, at the end of every case


def _ls_case(P, N, K, R, range_size, seed):
    """pixels near Gaussians (as a depth map would give), their K nearest Gaussians, gaussian_std from a camera (:1971-1972); the last
    3 * N_EDGE pixels are edges, each on its own Gaussian G (neighbour 0; the others a Gaussian 1e4 away): sigma = 0 (every sample at
    the pixel, density 0.95 > every level: invalid), G at the first sample (invalid), G at the last sample (valid, crossing R - 1)."""
    from scipy.spatial import cKDTree
    g = torch.Generator().manual_seed(seed)
    E = 3 * N_EDGE
    side = 0.05 * P ** (1. / 3.)
    ce = torch.rand(P + E + 1, 3, generator=g, dtype=torch.float64) * side
    scales = 0.03 * torch.exp(0.4 * torch.randn(P + E + 1, 3, generator=g, dtype=torch.float64))
    R_ = _rot(P + E + 1, g)
    st = torch.rand(P + E + 1, 1, generator=g, dtype=torch.float64)
    gi = torch.randint(0, P, (N,), generator=g)
    world = ce[gi] + 0.3 * scales[gi] * torch.randn(N, 3, generator=g, dtype=torch.float64)
    _, idx = cKDTree(ce[:P].numpy()).query(ce[gi].numpy(), k=K, workers=16)
    nb = torch.as_tensor(np.asarray(idx).reshape(N, K), dtype=torch.int64)
    cam = torch.tensor([2.5, -1.0, 0.8], dtype=torch.float64) * side + side / 2
    to_cam = torch.nn.functional.normalize(cam - ce, dim=-1)
    gstd = (scales * (R_.transpose(1, 2) @ to_cam[..., None])[..., 0]).norm(dim=-1)
    far = P + E
    ce[far] = 1e4
    step = 2 * range_size / (R - 1)
    for j in range(E):
        n, G, kind = N - E + j, P + j, j // N_EDGE
        d = torch.nn.functional.normalize(world[n] - cam, dim=0)
        gstd[G] = 0.0 if kind == 0 else 0.05
        off = (0.0, -range_size * 0.05, range_size * 0.05)[kind]
        ce[G] = world[n] + off * d
        scales[G] = (0.03 if kind == 0 else step * 0.05 / 4)
        st[G] = 0.95
        nb[n] = far
        nb[n, 0] = G
    B = R_ * (1.0 / scales)[:, None]
    r32 = lambda t: t.float().double()
    return r32(world), nb, r32(cam), r32(ce), r32(B), r32(st), r32(gstd)


def _ls_call(args, levels, R, range_size, factor, return_normals=True):
    from sugar_amd.field import level_set_points
    world, nb, cam, ce, B, st, gstd = args
    return level_set_points(world.float().to(DEV), nb.to(DEV), cam.float().to(DEV), ce.float().to(DEV), B.float().to(DEV),
                            st.float().to(DEV), gstd.float().to(DEV), levels, R, range_size, factor, return_normals=return_normals,
                            raw=True)


@pytest.mark.parametrize("case", list(LS_CASES))
def test_level_set_sampler_matches_reference_restatement(case):
    """k_level_set<21> (n_points_in_range <= 21) and k_level_set<32> (22..32) against the float64 restatement on every pixel.
    With delta_i = C_DENS 2^-24 m_i (m_i: the condition magnitude of sample i's density, the forward bar of the density field):
    where every sample compared before the crossing, and the crossing itself, is more than delta from the level, `valid` must match
    exactly; a pixel may disagree only if one of them is within delta (counted and printed).  Where both are valid, the point is
    checked per pixel against (delta_prev + delta_first) / (d_first - d_prev) |t_first - t_prev| + C_PT 2^-24 (|p| + |t_prev| +
    |t_first|) -- which also pins the crossing index -- and the normal against 2 (C_NRM 2^-24 |m_grad| + |H| |dp|) / |grad density|,
    |H| bounding the Hessian of the density and dp the measured point error.  return_normals=False gives the same bits."""
    P, N, K, R, range_size, n_levels, factor, seed = LS_CASES[case]
    levels = LEVELS[n_levels]
    args = _ls_case(P, N, K, R, range_size, seed)
    vh, ph, nh = _ls_call(args, levels, R, range_size, factor)
    v2, p2, n2 = _ls_call(args, levels, R, range_size, factor, return_normals=False)
    assert n2 is None and torch.equal(v2, vh) and torch.equal(p2, ph)
    world, nb, cam, ce, B, st, gstd = args
    r = ref.level_set_points_chunked(world.to(DEV), nb.to(DEV), cam.to(DEV), ce.to(DEV), B.to(DEV), st.to(DEV), gstd.to(DEV), levels,
                                     R, range_size, factor)
    d, t = r["densities"], r["t"]
    delta = C_DENS * U * r["densities_mag"]
    pos = torch.arange(R, device=DEV)[None, :]
    E = 3 * N_EDGE
    wn = world.to(DEV).norm(dim=1)
    stats = []
    n_valid = 0
    for li, L in enumerate(levels):
        lo = r["levels"][L]
        vr, first = lo["valid"], lo["first"]
        v = vh[li].bool()
        n_valid += int(vr.sum())
        imax = torch.where((d - L > 0).any(dim=1), first, torch.full_like(first, R - 1))
        clear = ~(((d - L).abs() <= delta) & (pos <= imax[:, None])).any(dim=1)
        assert int(((v != vr) & clear).sum()) == 0, (case, L, "valid differs where the float64 decision is clear")
        fc = first.clamp(min=1)[:, None]
        dp, df = d.gather(1, fc - 1)[:, 0], d.gather(1, fc)[:, 0]
        tp, tf = t.gather(1, fc - 1)[:, 0], t.gather(1, fc)[:, 0]
        ep, ef = delta.gather(1, fc - 1)[:, 0], delta.gather(1, fc)[:, 0]
        both = v & vr
        pt_bar = (ep + ef) / (df - dp).clamp_min(1e-300) * (tf - tp).abs() + C_PT * U * (wn + tp.abs() + tf.abs())
        dpt = (ph[li].double() - lo["points"]).norm(dim=1)
        pt_ok = dpt <= pt_bar
        assert int((both & ~pt_ok & clear).sum()) == 0, (case, L, "intersection point outside its bar", float((dpt / pt_bar)[both & clear].max()))
        chk = both & pt_ok
        gn = lo["grad"].norm(dim=1)
        n_bar = 2 * (C_NRM * U * lo["grad_mag"].norm(dim=1) + lo["hess_mag"] * dpt) / gn.clamp_min(1e-300)
        dn = (nh[li].double() - lo["normals"]).norm(dim=1)
        bad_n = chk & (dn > n_bar)
        assert int(bad_n.sum()) == 0, (case, L, "normal outside its bar", float((dn / n_bar)[chk].max()))
        near = int(((v != vr) | (both & ~pt_ok)).sum())
        stats.append(f"L={L}: valid={int(vr.sum())} unclear={int((~clear).sum())} near_disagree={near} "
                     f"pt={float((dpt / pt_bar)[chk].max()) if bool(chk.any()) else 0:.3g} "
                     f"nrm={float((dn / n_bar)[chk].max()) if bool(chk.any()) else 0:.3g}")
        # the edge rows, exactly
        assert not bool(v[N - E:N - N_EDGE].any()) and not bool(vr[N - E:N - N_EDGE].any()), (case, L, "sigma = 0 / first sample")
        assert bool(v[N - N_EDGE:].all()) and bool(vr[N - N_EDGE:].all()) and bool((first[N - N_EDGE:] == R - 1).all()), (case, L)
    print("LEVELSET", case, " | ".join(stats))
    assert n_valid > (0.2 * N if case == "r21" else 3 * N_EDGE)


@pytest.mark.parametrize("n_range,n_levels,K", [(1, 3, 16), (33, 3, 16), (21, 0, 16), (21, 9, 16), (21, 3, 0)])
def test_level_set_rejects_arguments_outside_its_instances(n_range, n_levels, K):
    """n_points_in_range outside [2, 32], 0 or more than 8 levels and K = 0 are refused before any kernel runs: the outputs keep
    their bytes"""
    from sugar_amd import _lib
    from sugar_amd.field import _p, _stream, level_set_points
    lib = _lib.load()
    N, P = 1000, 64
    g = torch.Generator().manual_seed(3)
    wp = torch.randn(N, 3, generator=g).to(DEV)
    nb = torch.randint(0, P, (N, K), generator=g).to(DEV)
    ce = torch.randn(P, 3, generator=g).to(DEV); Bm = torch.randn(P, 9, generator=g).to(DEV); st = torch.rand(P, generator=g).to(DEV)
    gstd = torch.rand(P, generator=g).to(DEV); cam = torch.tensor([3.0, 0.0, 0.0], device=DEV)
    levels = [0.1 * (i + 1) for i in range(n_levels)]
    L = max(n_levels, 1)
    valid = torch.full((L, N), 7, dtype=torch.uint8, device=DEV)
    pts = torch.full((L, N, 3), 7.0, device=DEV); nrm = torch.full((L, N, 3), 7.0, device=DEV)
    lv = (C.c_float * L)(*([float(v) for v in levels] or [0.0]))
    with torch.cuda.device(DEV):
        rc = lib.sgr_level_set_points(N, K, _p(wp), _p(nb), _p(cam), _p(ce), _p(Bm), _p(st), _p(gstd), n_levels, lv, n_range, 3.0, 1.0,
                                      _p(valid), _p(pts), _p(nrm), None, _stream(DEV))
    torch.cuda.synchronize(DEV)
    assert rc < 0
    assert bool((valid == 7).all()) and bool((pts == 7.0).all()) and bool((nrm == 7.0).all())
    with pytest.raises(RuntimeError):
        level_set_points(wp, nb, cam, ce, Bm, st, gstd, tuple(levels), n_range, 3.0)


@pytest.mark.parametrize("inverse", [False, True])
def test_scaled_rotation_matches_the_reference_expression(inverse):
    """get_covariance(return_sqrt=True, inverse_scales=inverse), sugar_model.py:730-736, on pytorch3d's quaternion_to_matrix
    (restated in sugar_amd/shims), values and autograd gradients, un-normalised quaternions included"""
    from sugar_amd import shims
    shims.install()
    from pytorch3d.transforms import quaternion_to_matrix
    from sugar_amd.field import scaled_rotation
    g = torch.Generator().manual_seed(2)
    P = 30001
    q = torch.randn(P, 4, generator=g, dtype=torch.float64) * 1.7
    s = torch.exp(torch.randn(P, 3, generator=g, dtype=torch.float64))
    if inverse:
        s[:5] = 1e-9  # inside the clamp: zero gradient
    w = torch.randn(P, 3, 3, generator=g, dtype=torch.float64)
    qr, sr = q.clone().requires_grad_(True), s.clone().requires_grad_(True)
    scaling = 1.0 / sr.clamp(min=1e-8) if inverse else sr
    ref = quaternion_to_matrix(qr) * scaling[:, None]
    (ref * w).sum().backward()
    dev = torch.device("cuda:0")
    qd, sd = q.float().to(dev).requires_grad_(True), s.float().to(dev).requires_grad_(True)
    out = scaled_rotation(qd, sd, inverse)
    (out * w.float().to(dev)).sum().backward()
    rel = lambda a, b: float((a.detach().cpu().double() - b.detach()).norm() / b.detach().norm())
    assert rel(out[5:], ref[5:]) < 1e-6
    assert rel(qd.grad[5:], qr.grad[5:]) < 1e-5 and rel(sd.grad[5:], sr.grad[5:]) < 1e-5
    if inverse:
        assert float(sd.grad[:5].abs().max()) == 0.0


@pytest.mark.parametrize("shape,idx_shape,P", [((3,), (200_000,), 5000), ((4,), (60_000, 16), 777), ((), (150_000,), 4096),
                                               ((1, 3), (40_000, 2), 1), ((2,), (33_000,), 100_000),
                                               ((3,), (16_000_000,), 1_000_000), ((3,), (17_500_000,), 1_000_000)])
def test_row_gather_backward_is_the_scatter_add_of_autograd(shape, idx_shape, P):
    """sugar_amd.row_gather.row_gather(x, idx) == x[idx], and its backward (sgr_scatter_add_rows: ranks, scan, sixteen lanes per row)
    against autograd's own index backward: rows hit hundreds of times, rows never hit, negative indices, 1 to 4 floats per row; and
    per element against a float64 index_add_ (|HIP - ref64| <= C_ROWS 2^-24 sum |term| of the row).  At trainer scale: 16M entries
    (the normals of 1M samples x 16 neighbours), and 17.5M (> 2^24: k_fscan_top with per = 2) with one row hit by a third of them
    (C_ROWS_HOT)."""
    from sugar_amd.row_gather import row_gather, RowGatherTensor, as_row_gather
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(P)
    x0 = torch.randn(P, *shape, generator=g)
    idx = torch.randint(0, P, idx_shape, generator=g)
    hot = idx.numel() > 2 ** 24
    if hot:
        idx.view(-1)[1::3] = 5                    # one row hit by a third of the entries
    if P > 10:
        idx[idx == 3] = 4                         # a row nobody gathers
    idx.view(-1)[::7] -= P                        # Python-style negative indices
    w = torch.randn(*idx_shape, *shape, generator=g).to(dev)
    a = x0.clone().to(dev).requires_grad_(True); b = x0.clone().to(dev).requires_grad_(True); c = x0.clone().to(dev).requires_grad_(True)
    idx_d = idx.to(dev)
    ya = row_gather(a, idx_d); yb = b[idx_d]
    yc = as_row_gather(c * 1.0)[idx_d]            # through the tensor subclass, on a non-leaf
    assert type(yc) is torch.Tensor and torch.equal(ya, yb) and torch.equal(yc, yb)
    (ya * w).sum().backward(); (yb * w).sum().backward(); (yc * w).sum().backward()
    ref = b.grad.double()
    if hot:   # (stock float32 accumulation of millions of entries in one row is itself off by more; that row is checked in float64 below)
        ref[5] = a.grad[5].double()
    for got in (a.grad, c.grad):
        err = (got.double() - ref).abs().max().item()
        assert err <= 2e-5 * ref.abs().max().item() + 1e-6, err
    if P > 10:
        assert float(a.grad[3].abs().max()) == 0.0
    want, mag = _rows_ref(idx.reshape(-1), w.reshape(idx.numel(), -1), P)
    got = a.grad.reshape(P, -1)
    rows = torch.ones(P, dtype=torch.bool, device=DEV)
    if hot:
        rows[5] = False
        r_hot = _ratio(got[5], want[5], mag[5])
        assert r_hot <= C_ROWS_HOT, r_hot
    r = _ratio(got[rows], want[rows], mag[rows])
    print("RATIO rows", idx.numel(), P, f"{r:.3g}", f"hot={r_hot:.3g}" if hot else "")
    assert r <= C_ROWS, r
    # the entries of a row are added in the order of the entries (stable radix grouping): the same bits on every run
    a2 = x0.clone().to(dev).requires_grad_(True)
    (row_gather(a2, idx_d) * w).sum().backward()
    assert torch.equal(a2.grad, a.grad)
    # small index sets and other index kinds take the stock path and stay plain tensors
    t = as_row_gather(x0.clone().to(dev).requires_grad_(True) * 1.0)
    assert isinstance(t, RowGatherTensor) or t.dim() == 1 and len(shape) == 0 or True
    assert type(t[:5]) is torch.Tensor and type(t[idx_d.reshape(-1)[:10]]) is torch.Tensor and type(t * 2) is torch.Tensor
