"""tests/sdm_ref.py, the numpy restatement that the signed-distance and edge kernels are held to, pinned to the reference's own
functions: to tests/golden/sdm_edge.npz (written by tests/golden/make_golden_sdm.py from the reference's `convert_labels`, `edge_3d`
and `compute_sdf`) and, where skimage is installed, to the real `find_boundaries(mode='inner')`."""
import os

import numpy as np
import pytest

from tests import sdm_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdm_edge.npz")


def fixture_labels():
    from tests import sdm_checks as C
    return C.fixture_labels()


def test_restatement_equals_the_reference_on_the_fixture():
    g = np.load(GOLDEN)
    labels = fixture_labels()
    assert np.array_equal(g["labels"], labels) and g["labels"].dtype == np.int16
    seg = S.convert_labels(labels)
    assert seg.shape == (1, 3, 9, 10, 24) and np.array_equal(seg, g["seg"])
    edge, sdf, sdm = S.targets(labels[None])
    assert np.array_equal(edge, g["edge"])
    assert sdf.dtype == np.float64 and np.array_equal(sdf, g["sdf"]) and np.array_equal(sdm, g["sdm"])
    assert np.array_equal(S.edge_3d(seg), g["edge"]) and np.array_equal(S.compute_sdf(seg, seg.shape), g["sdf"])


def test_fixture_properties():
    """what the case was chosen for: every region passes the reference's asserts; WT touches two faces, so edge and inner boundary
    differ; sdm spans [0, 2.75]"""
    g = np.load(GOLDEN)
    assert all(S.asserts_hold(g["sdf"][0, r]) for r in range(3))
    wt = g["seg"][0, 1].astype(bool)
    edge, bnd = g["edge"][0, 1].astype(bool), S.find_boundaries_inner(wt)
    assert int(edge.sum()) == 568 and int(bnd.sum()) == 554 and int((edge & ~bnd).sum()) == 14 and not (bnd & ~edge).any()
    assert float(g["sdm"].min()) == 0.0 and float(g["sdm"].max()) == 2.75
    assert not g["seg"][:, :, 8, 9, 0].any()                              # the voxel of -1 is in no region


def test_full_and_empty_and_thin_regions():
    full = np.ones((3, 4, 5), bool)
    assert not S.sdf_of_mask(full).any() and not S.sdf_of_mask(~full).any()
    with np.errstate(all="ignore"):
        assert np.isnan(S.sdf_of_mask(full, full_is_zero=False)).all()    # the reference's 0 / 0
    slab = np.zeros((6, 7, 9), bool)
    slab[2:4] = True
    sdf = S.sdf_of_mask(slab)
    assert not S.asserts_hold(sdf) and sdf.min() == 0.0 and sdf.max() == 1.0


def test_inner_boundary_equals_skimage():
    seg = pytest.importorskip("skimage.segmentation")
    rng = np.random.RandomState(0)
    for shape in ((9, 10, 24), (5, 6, 7), (1, 1, 1), (12, 13)):
        for p in (0.2, 0.5, 0.9, 1.0):
            m = rng.rand(*shape) < p
            assert np.array_equal(S.find_boundaries_inner(m), seg.find_boundaries(m, mode="inner"))
    wt = np.load(GOLDEN)["seg"][0, 1].astype(bool)
    assert np.array_equal(S.find_boundaries_inner(wt), seg.find_boundaries(wt, mode="inner"))
