"""Device-side case preparation (segmamba_amd/preprocess.py) on the HIP library: the checks of tests/test_emu_preprocess.py on the GPU,
plus the case at BraTS size (155 x 240 x 240 x 4), whose hole filling is referenced by the label propagation written with plain ATen
ops on the device (tests/postprocess_checks.py `torch_fill`; no scipy needed)."""
import numpy as np
import pytest
import torch

from tests import postprocess_checks as PK
from tests import preprocess_checks as K
from tests import preprocess_ref as R
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"

# conditions on the BraTS-size input, computed with numpy / scipy on the host when the case was written
BRATS_BOX = [[21, 140], [41, 210], [49, 188]]
BRATS_FILL_ADDS = 39984


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("shape", [(37, 46, 53), (21, 26, 30)])
def test_brain_mask_box_crop(hip, shape):
    K.check_brain_crop(hip, DEV, shape)


def test_odd_shapes_and_strided_views(hip):
    K.check_shapes_and_strides(hip, DEV)


def test_faces_single_voxel_nan_no_seg_int16(hip):
    K.check_further_cases(hip, DEV)


def test_normalisation(hip):
    K.check_normalisation(hip, DEV)


def test_class_locations(hip):
    K.check_class_locations(DEV)


def test_preprocess_case_end_to_end(hip):
    data, seg, info = R.brain_case((37, 46, 53))
    K.check_preprocess_case(hip, DEV, data, seg, info)


def test_case_preprocessor_files(hip, tmp_path):
    K.check_case_preprocessor(DEV, tmp_path)


def test_refusals(hip):
    K.check_refusals(hip, DEV)


def test_new_exports(hip):
    K.check_exports(hip)


def _device_fill(mask):
    return PK.torch_fill(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)).bool().cpu().numpy()


def test_preprocess_case_at_brats_size(hip):
    """the whole of `preprocess_case` at 155 x 240 x 240 x 4 against the restatement: box, seg, class locations exactly, the
    normalisation within the fp32 bound, and back through `labels_from_logits`"""
    data, seg, info = R.brats_case()
    assert data.shape == (4, 155, 240, 240)
    K.check_preprocess_case(hip, DEV, data, seg, info, fill_fn=_device_fill, expect_box=BRATS_BOX, expect_added=BRATS_FILL_ADDS)


def test_masked_normalisation_at_brats_size(hip):
    from segmamba_amd import preprocess as P
    data, seg, info = R.brats_case()
    d, s = P.preprocess_case(K.dev_t(data, DEV), K.dev_t(seg, DEV), {"spacing": (1.0, 1.0, 1.0)}, use_mask_for_norm=True)
    want = R.run_case(data, seg, (1.0, 1.0, 1.0), mask_norm=True, fill_fn=_device_fill)
    assert want[2]["bbox_used_for_cropping"] == BRATS_BOX and np.array_equal(s.cpu().numpy(), want[1])
    inside = want[1][0] >= 0
    assert inside.any() and (~inside).any()
    sl = (slice(None),) + tuple(slice(a, b) for a, b in BRATS_BOX)
    raw_crop = np.ascontiguousarray(data[sl])
    got = d.cpu().numpy()
    for c in range(4):
        K._norm_within(got[c], raw_crop[c], inside, name=f"BraTS size, masked channel {c}")
