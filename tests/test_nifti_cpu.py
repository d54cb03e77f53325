"""segmamba_amd/nifti.py (host only), Predictor.save_to_nii on the emulated library, and the two tools end to end:
tools/finish_predictions.py then tools/compute_metrics.py."""
import gzip
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from segmamba_amd import nifti
from tests import emu_util
from tests import metrics_ref as MR
from tests import postprocess_ref as R
from segmamba_amd import lib as L

needs_emu = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture
def product(monkeypatch):
    emu = emu_util.emu_lib()
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def _array(dtype, shape, seed=0):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.standard_normal(shape).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=shape, endpoint=True).astype(dtype)


@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.float32])
def test_round_trip(tmp_path, dtype, ext):
    for shape in ((5, 7, 3), (1, 1, 1), (2, 31, 17)):
        a = _array(dtype, shape)
        path = str(tmp_path / f"v_{shape[0]}{ext}")
        nifti.write_nifti(path, a, (0.5, 1.25, 3.0))
        b, spacing = nifti.read_nifti(path)
        assert b.dtype == np.dtype(dtype) and np.array_equal(a, b)
        assert spacing == (0.5, 1.25, 3.0)
    # a view that is not contiguous, and bool
    a = _array(dtype, (4, 6, 8))[:, ::2, 1:]
    nifti.write_nifti(str(tmp_path / f"view{ext}"), a)
    assert np.array_equal(nifti.read_nifti(str(tmp_path / f"view{ext}"))[0], a)
    nifti.write_nifti(str(tmp_path / f"bool{ext}"), a != 0)
    got = nifti.read_nifti(str(tmp_path / f"bool{ext}"))[0]
    assert got.dtype == np.uint8 and np.array_equal(got, (a != 0).astype(np.uint8))


def test_header_fields_from_the_raw_bytes(tmp_path):
    a = _array(np.int16, (4, 5, 6))                      # (z, y, x)
    path = str(tmp_path / "h.nii.gz")
    nifti.write_nifti(path, a, (0.75, 1.5, 2.0))         # spacing in the order given: pixdim[1..3]
    raw = gzip.open(path, "rb").read()
    assert len(raw) == 352 + a.size * 2
    assert struct.unpack_from("<i", raw, 0)[0] == 348                                   # sizeof_hdr
    assert struct.unpack_from("<8h", raw, 40) == (3, 6, 5, 4, 1, 1, 1, 1)               # dim = [3, X, Y, Z, 1, 1, 1, 1]
    assert struct.unpack_from("<hh", raw, 70) == (4, 16)                                # datatype, bitpix
    assert struct.unpack_from("<4f", raw, 76) == (1.0, 0.75, 1.5, 2.0)                  # qfac, pixdim[1..3]
    assert struct.unpack_from("<f", raw, 108)[0] == 352.0                               # vox_offset
    assert struct.unpack_from("<ff", raw, 112) == (1.0, 0.0)                            # scl_slope, scl_inter
    assert struct.unpack_from("<hh", raw, 252) == (1, 1)                                # qform_code, sform_code
    assert struct.unpack_from("<6f", raw, 256) == (0.0, 0.0, 1.0, 0.0, 0.0, 0.0)        # quaternion (b, c, d), zero origin
    assert struct.unpack_from("<4f", raw, 280) == (-0.75, 0.0, 0.0, 0.0)                # srow_x
    assert struct.unpack_from("<4f", raw, 296) == (0.0, -1.5, 0.0, 0.0)                 # srow_y
    assert struct.unpack_from("<4f", raw, 312) == (0.0, 0.0, 2.0, 0.0)                  # srow_z
    assert raw[344:348] == b"n+1\0" and raw[348:352] == b"\0\0\0\0"
    # x is the fastest axis on disk
    assert np.array_equal(np.frombuffer(raw, "<i2", offset=352).reshape(4, 5, 6), a)
    codes = {np.uint8: (2, 8), np.int32: (8, 32), np.float32: (16, 32)}
    for dt, want in codes.items():
        nifti.write_nifti(str(tmp_path / "t.nii"), _array(dt, (2, 2, 2)))
        assert struct.unpack_from("<hh", open(tmp_path / "t.nii", "rb").read(), 70) == want


def test_refusals(tmp_path):
    a = np.zeros((2, 3, 4), np.uint8)
    for bad in (lambda: nifti.write_nifti(str(tmp_path / "a.nii"), a.astype(np.float64)),
                lambda: nifti.write_nifti(str(tmp_path / "a.nii"), a[0]),
                lambda: nifti.write_nifti(str(tmp_path / "a.img"), a),
                lambda: nifti.write_nifti(str(tmp_path / "a.nii"), a, (1, 0, 1)),
                lambda: nifti.write_nifti(str(tmp_path / "a.nii"), a, (1, 1))):
        with pytest.raises(RuntimeError):
            bad()
    good = str(tmp_path / "good.nii")
    nifti.write_nifti(good, a)
    raw = bytearray(open(good, "rb").read())

    def variant(name, edit):
        b = bytearray(raw)
        edit(b)
        open(tmp_path / name, "wb").write(bytes(b))
        return str(tmp_path / name)
    cases = [variant("scaled.nii", lambda b: struct.pack_into("<ff", b, 112, 2.0, 1.0)),
             variant("float64.nii", lambda b: struct.pack_into("<hh", b, 70, 64, 64)),
             variant("pair.nii", lambda b: b.__setitem__(slice(344, 348), b"ni1\0")),
             variant("ext.nii", lambda b: b.__setitem__(348, 1)),
             variant("bigendian.nii", lambda b: struct.pack_into(">i", b, 0, 348)),
             variant("fourd.nii", lambda b: struct.pack_into("<8h", b, 40, 4, 4, 3, 2, 2, 1, 1, 1)),
             variant("short.nii", lambda b: b.__delitem__(slice(360, None)))]
    for path in cases:
        with pytest.raises(RuntimeError):
            nifti.read_nifti(path)
    slope0 = variant("slope0.nii", lambda b: struct.pack_into("<ff", b, 112, 0.0, 0.0))       # scl_slope 0 = unscaled
    assert np.array_equal(nifti.read_nifti(slope0)[0], a)


@needs_emu
def test_save_to_nii_emulated(product, tmp_path):
    """the reference's call (prediction.py:208-227) on the drop-in class: labels, then a mask with postprocess = True"""
    from segmamba_amd.predictor import Predictor
    pred, _ = MR.small_case((20, 30, 25))
    p = Predictor(window_infer=None, mirror_axes=[0, 1, 2])
    path = p.save_to_nii(torch.from_numpy(pred), [torch.tensor(1.0), torch.tensor(0.9), torch.tensor(2.5)], str(tmp_path / "out"), "case_a")
    assert path.endswith("case_a.nii.gz") and os.path.exists(path)
    got, spacing = nifti.read_nifti(path)
    assert np.array_equal(got, pred) and spacing == (1.0, float(np.float32(0.9)), 2.5)
    wt = MR.region_mask(pred, (1, 2, 3))
    p.save_to_nii(wt, (1, 1, 1), str(tmp_path / "out"), "case_b", postprocess=True)          # numpy bool in, as the reference's astype
    got, _ = nifti.read_nifti(str(tmp_path / "out" / "case_b.nii.gz"))
    assert got.dtype == np.uint8 and np.array_equal(got, R.largest_connected_domain(wt))
    assert int(wt.sum()) - int(got.sum()) == 8                                                # the false-positive island went
    p.save_to_nii(torch.from_numpy(pred)[None], (1, 1, 1), str(tmp_path / "out"), "case_c")  # (1, D, H, W)
    assert np.array_equal(nifti.read_nifti(str(tmp_path / "out" / "case_c.nii.gz"))[0], pred)
    with pytest.raises(RuntimeError, match="one file per channel"):
        p.save_to_nii(np.stack([wt, wt, wt]), (1, 1, 1), str(tmp_path / "out"), "case_d")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(emu_util.ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@needs_emu
def test_finish_predictions_then_compute_metrics_emulated(product, tmp_path):
    """.npy / .npz logits -> .nii.gz labels -> the metrics of the in-memory path"""
    finish, compute = _tool("finish_predictions"), _tool("compute_metrics")
    for d in ("logits", "gt"):
        (tmp_path / d).mkdir()
    want, labels = [], {}
    for i in range(2):
        pred, gt = MR.small_case((20 + i, 30, 25))
        onehot = np.stack([(pred == c) for c in range(4)]).astype(np.float32) * 3.0
        if i == 0:
            np.save(tmp_path / "logits" / "case0.npy", onehot)
            full = pred
        else:                                               # with properties: pasted into a larger volume
            shape = (25, 33, 30)
            box = [[2, 2 + pred.shape[0]], [1, 1 + pred.shape[1]], [4, 4 + pred.shape[2]]]
            np.savez(tmp_path / "logits" / "case1.npz", logits=onehot, shape_after_cropping_before_resample=np.array(pred.shape),
                     bbox_used_for_cropping=np.array(box), shape_before_cropping=np.array(shape), spacing=np.array([1.0, 1.0, 1.0]))
            full = R.paste(pred, shape, (2, 1, 4))
            gt = R.paste(gt, shape, (2, 1, 4))
        labels[i] = full
        nifti.write_nifti(str(tmp_path / "gt" / f"case{i}.nii.gz"), gt)
        want.append(MR.case_metrics(full, gt))
    written = finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / "pred")])
    assert [os.path.basename(w) for w in written] == ["case0.nii.gz", "case1.nii.gz"]
    for i in range(2):
        assert np.array_equal(nifti.read_nifti(written[i])[0], labels[i])
    res = compute.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt")])
    assert res.shape == (2, 3, 2) and np.allclose(res, np.stack(want), rtol=1e-6, atol=0.0)
    written = finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / "pp"), "--postprocess"])
    assert np.array_equal(nifti.read_nifti(written[0])[0], R.postprocess_labels(labels[0]))


def test_reads_back_through_nibabel_or_simpleitk(tmp_path):
    """where either library imports, the file written here reads back equal through it (neither is installed where this was written:
    unverified there)"""
    a = _array(np.uint8, (4, 5, 6))
    path = str(tmp_path / "x.nii.gz")
    nifti.write_nifti(path, a, (0.5, 1.0, 2.0))
    try:
        sitk = pytest.importorskip("SimpleITK")
        img = sitk.ReadImage(path)
        assert np.array_equal(sitk.GetArrayFromImage(img), a) and tuple(img.GetSpacing()) == (0.5, 1.0, 2.0)
    except pytest.skip.Exception:
        nib = pytest.importorskip("nibabel")
        img = nib.load(path)
        assert np.array_equal(np.asarray(img.dataobj).transpose(2, 1, 0), a)
