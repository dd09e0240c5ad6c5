"""CPU tests of the refined-mesh postprocess: the yardstick (tests/mesh_postprocess_restatement.py) against an independent brute-force
statement of the reference's own criterion, the properties of the peel rule, the condition the re-add case must meet for a float32
implementation to be comparable, and the parts of sugar_amd.mesh_postprocess / sugar_amd.refined_mesh that need no GPU: argument errors,
the command-line parser, the checkpoint reader, the ABI table."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import mesh_postprocess_restatement as mpr  # noqa: E402

CASES = {"sheet12x9+extras": lambda: mpr.with_extras(mpr.sheet(12, 9)), "sheet7x5+extras": lambda: mpr.with_extras(mpr.sheet(7, 5)),
         "sheet7x5": lambda: mpr.sheet(7, 5), "octahedron": lambda: mpr.octahedron(2)[1]}


# ---------------------------------------------------------------- both formulations agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_slot_counting_equals_the_reference_criterion(name):
    faces = CASES[name]()
    for it in range(7):
        assert np.array_equal(mpr.peel(faces, it), mpr.peel_reference_criterion(faces, it)), (name, it)
    m0 = mpr.initial_mask(len(faces))
    for it in (1, 3):
        assert np.array_equal(mpr.peel(faces, it, m0), mpr.peel_reference_criterion(faces, it, m0)), (name, it)


def test_live_counts_of_the_issue():
    """the counts both formulations gave when the rule was written down"""
    faces = CASES["sheet12x9+extras"]()
    assert [int(mpr.peel(faces, it).sum()) for it in range(7)] == [220, 181, 145, 112, 83, 58, 38]
    small = CASES["sheet7x5+extras"]()
    assert len(small) == 74
    for it in (5, 6, 9):
        live = mpr.peel(small, it)
        assert np.nonzero(live)[0].tolist() == [71, 72]        # the duplicated pair


# ---------------------------------------------------------------- peel properties
def test_a_closed_surface_loses_nothing():
    verts, faces = mpr.octahedron(2)
    assert len(faces) == 128
    assert mpr.peel(faces, 9).all()


def test_a_sheet_loses_a_ring_per_iteration_and_empties():
    nx, ny = 7, 5
    faces = mpr.sheet(nx, ny)
    cell = np.repeat(np.arange(nx * ny), 2)
    ci, cj = cell % nx, cell // nx
    ring = np.minimum(np.minimum(ci, nx - 1 - ci), np.minimum(cj, ny - 1 - cj))     # the cell's distance to the rim
    prev = np.ones(len(faces), bool)
    for it in range(1, 10):
        live = mpr.peel(faces, it)
        assert not (live & ~prev).any()                          # nothing comes back
        assert not live[ring < (it - 1) // 2].any()              # a ring of cells is gone after two steps (one triangle per step) ...
        assert live[ring >= it].all()                            # ... and no step reaches deeper than one cell
        prev = live
    assert mpr.peel(faces, 2).sum() < mpr.peel(faces, 1).sum() < len(faces)
    assert not mpr.peel(faces, 3)[ring == 0].any()
    assert not mpr.peel(faces, 9).any() and not mpr.peel(faces, 12).any()           # empty stays empty


def test_counts_are_over_slots():
    # three faces around one edge {0,1}: the edge counts 3, the six outer edges 1 -> all die at once
    fan = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    assert not mpr.peel(fan, 1).any()
    # a closed tetrahedron plus a third face on its edge {0,1}: that edge counts 3 (fine), the new face's outer edges 1
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0], [0, 1, 4]])
    assert mpr.peel(tet, 1).tolist() == [True, True, True, True, False]
    assert mpr.peel(tet, 5).tolist() == [True, True, True, True, False]
    # two copies of one face keep each other alive for ever; a single copy dies
    assert mpr.peel(np.array([[0, 1, 2], [0, 1, 2]]), 9).all()
    assert mpr.peel(np.array([[2, 1, 0], [0, 1, 2]]), 9).all()             # orientation does not matter: pairs are unordered
    assert not mpr.peel(np.array([[0, 1, 2]]), 1).any()
    # (i, j, j): {i,j} counts 2 by itself, {j,j} counts 1 -> it dies alone, but it lends {i,j} two counts while it lives
    assert not mpr.peel(np.array([[0, 1, 1]]), 1).any()
    assert mpr.peel(np.array([[0, 1, 1], [0, 1, 1]]), 9).all()             # {1,1} now counts 2
    # a given initial mask is honoured: killing one copy of the pair kills the other in one step, and dead faces stay dead
    pair = np.array([[0, 1, 2], [0, 1, 2]])
    assert mpr.peel(pair, 0, [True, False]).tolist() == [True, False]
    assert mpr.peel(pair, 1, [True, False]).tolist() == [False, False]
    verts, faces = mpr.octahedron(2)
    m0 = np.ones(len(faces), bool)
    m0[17] = False
    out = mpr.peel(faces, 1, m0)
    assert not out[17] and out.sum() == len(faces) - 1 - 3                 # the hole's three neighbours go


# ---------------------------------------------------------------- the re-add case
def test_readd_case_is_decidable_in_float32():
    """every dead face's float64 density lies outside threshold (1 +- 1e-3) -- three orders above the float32 error of a 16-term sum --
    with no face exempted, and the case has both outcomes"""
    c = mpr.readd_case()
    dens = mpr.face_density(c["verts"], c["faces"], c["points"], c["scaling"], c["quaternions"], c["strengths"])
    dead = ~c["mask"]
    assert dead.sum() >= 20
    assert mpr.margin_ok(c["mask"], dens, c["threshold"])
    out = mpr.readd(c["mask"], dens, c["threshold"])
    assert (out & dead).any() and (~out & dead).any()
    assert np.array_equal(out[c["mask"]], c["mask"][c["mask"]])
    # no ties among the 16 nearest of any face centre
    centres = c["verts"].astype(np.float64)[c["faces"]].mean(1)
    d2 = np.sort(((centres[:, None] - c["points"].astype(np.float64)[None]) ** 2).sum(-1), axis=1)[:, :17]
    assert (np.diff(d2, axis=1) > 1e-9).all()


def test_compaction_keeps_the_rows_of_the_kept_faces():
    t = np.arange(4 * 3 * 2).reshape(12, 2)
    out = mpr.compact_rows(t, [True, False, False, True], 3)
    assert out.tolist() == t[[0, 1, 2, 9, 10, 11]].tolist()
    assert mpr.compact_rows(t, [False] * 4, 3).shape == (0, 2)


# ---------------------------------------------------------------- errors of the product that need no GPU
def test_cpu_tensors_raise():
    from sugar_amd import mesh_postprocess as mp
    faces = torch.from_numpy(mpr.sheet(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.peel_border_faces(faces, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.PeelTopology(faces)
    v = torch.zeros(12, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.readd_dense_faces(v, faces, torch.ones(12, dtype=torch.bool), torch.zeros(20, 3), torch.ones(20, 3), torch.ones(20, 4),
                             torch.ones(20), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.postprocess_bound_mesh(v, faces, 1, torch.zeros(12, 2), torch.ones(12, 2), torch.zeros(12, 1), 0.02)


def test_bad_arguments_raise_value_errors():
    from sugar_amd import mesh_postprocess as mp
    faces = torch.from_numpy(mpr.sheet(3, 2))
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        mp.peel_border_faces(faces.reshape(-1), 1)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        mp.peel_border_faces(faces[:, :2], 1)
    with pytest.raises(ValueError, match="int32 / int64"):
        mp.peel_border_faces(faces.float(), 1)
    with pytest.raises(ValueError, match="negative"):
        mp.peel_border_faces(faces, -1)
    with pytest.raises(ValueError, match="face_mask"):
        mp.peel_border_faces(faces, 1, face_mask=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="face_mask"):
        mp.peel_border_faces(faces, 1, face_mask=torch.ones(12, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"outside \[0, 11\)"):
        mp.peel_border_faces(faces, 1, n_verts=11)                # the sheet names vertex 11
    bad = faces.clone()
    bad[4, 1] = -1
    with pytest.raises(ValueError, match="outside"):
        mp.peel_border_faces(bad, 1)
    with pytest.raises(ValueError, match="1, 3, 4 and 6"):
        mp.bary_coords(2)
    for n in (1, 3, 4, 6):
        b = mp.bary_coords(n)
        assert b.shape == (n, 3) and torch.allclose(b.sum(1), torch.ones(n))


def test_cli_parser():
    from sugar_amd import refined_mesh as rm
    a = rm.parser().parse_args(["ck.pt", "--cameras", "c.json", "--out", "m.obj"])
    assert (a.checkpoint, a.cameras, a.out, a.square_size, a.postprocess, a.postprocess_iterations, a.postprocess_density_threshold,
            a.device) == ("ck.pt", "c.json", "m.obj", 10, False, 5, 0.1, "cuda:0")
    a = rm.parser().parse_args(["ck.pt", "--cameras", "c.json", "--out", "m.obj", "--square-size", "4", "--postprocess",
                                "--postprocess-iterations", "2", "--postprocess-density-threshold", "0.3", "--device", "cuda:1"])
    assert (a.square_size, a.postprocess, a.postprocess_iterations, a.postprocess_density_threshold, a.device) == (4, True, 2, 0.3, "cuda:1")
    for argv in (["--cameras", "c.json", "--out", "m.obj"], ["ck.pt", "--out", "m.obj"], ["ck.pt", "--cameras", "c.json"],
                 ["ck.pt", "--cameras", "c.json", "--out", "m.obj", "--square-size", "x"],
                 ["ck.pt", "--cameras", "c.json", "--out", "m.obj", "--postprocess", "yes"]):
        with pytest.raises(SystemExit):
            rm.parser().parse_args(argv)
    with pytest.raises(ValueError, match="square-size"):
        rm.main(["ck.pt", "--cameras", "c.json", "--out", "m.obj", "--square-size", "2"])


def test_checkpoint_reader(tmp_path):
    from sugar_amd import refined_mesh as rm
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in mpr.bound_case(4, 3, 3, seed=2).items()}
    m = rm.model_from_state_dict(sd)
    assert m["n"] == 3 and m["faces"].dtype == torch.int64 and m["verts"].shape == (20, 3) and m["all_densities"].shape == (72, 1)
    path = tmp_path / "ck.pt"
    torch.save({"epoch": 3, "state_dict": sd}, path)
    assert rm.load_checkpoint(str(path))["n"] == 3
    for k in rm.CHECKPOINT_KEYS:
        with pytest.raises(ValueError, match=re.escape(f"`{k}`")):
            rm.model_from_state_dict({q: v for q, v in sd.items() if q != k})
    with pytest.raises(ValueError, match="not F\\*n"):
        rm.model_from_state_dict({**sd, "_scales": sd["_scales"][:-1]})
    with pytest.raises(ValueError, match="not F\\*n"):                              # n = 2 does not exist
        rm.model_from_state_dict({**sd, "_scales": sd["_scales"][:48]})
    with pytest.raises(ValueError, match="disagree"):
        rm.model_from_state_dict({**sd, "all_densities": sd["all_densities"][:24]})
    torch.save({"model": 1}, path)
    with pytest.raises(ValueError, match="state_dict"):
        rm.load_checkpoint(str(path))


# ---------------------------------------------------------------- ABI
def test_abi_lists_the_new_entry_points(hip_lib):
    from sugar_amd import _lib
    header = open(os.path.join(ROOT, "include", "sugar_raster.h")).read()
    for name in ("sgr_mesh_peel_border", "sgr_mesh_peel_border_scratch_bytes"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header) and hasattr(hip_lib, name)
    assert hip_lib.sgr_abi_version() == _lib.ABI_VERSION == 4
    assert hip_lib.sgr_mesh_peel_border_scratch_bytes(0) == 0 and hip_lib.sgr_mesh_peel_border_scratch_bytes(1000) >= 1000
    # argument checks come before any launch: no GPU is needed for these
    assert hip_lib.sgr_mesh_peel_border(0, 0, None, None, None, 5, None, None, None) == 0          # F == 0: a no-op
    assert hip_lib.sgr_mesh_peel_border(10, 12, None, None, None, 0, None, None, None) == 0        # iterations == 0: a no-op
    assert hip_lib.sgr_mesh_peel_border(-1, 0, None, None, None, 1, None, None, None) == -1
    assert hip_lib.sgr_mesh_peel_border(10, 12, None, None, None, -1, None, None, None) == -1
    assert hip_lib.sgr_mesh_peel_border(10, 12, None, None, None, 1, None, None, None) == -1       # null pointers
    assert b"null pointer" in hip_lib.sgr_last_error()
    assert hip_lib.sgr_mesh_peel_border(10, 31, None, None, None, 1, None, None, None) == -1       # E > 3 F
    assert hip_lib.sgr_mesh_peel_border(1 << 29, 5, None, None, None, 1, None, None, None) == -1   # 3 F >= 2^30
