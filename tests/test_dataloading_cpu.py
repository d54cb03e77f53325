"""The patch loader (segmamba_amd/dataloading.py) on the host: keys and boxes equal to what the reference's own
`DataLoaderMultiProcess` drew under the same `np.random.seed` (tests/golden/patch_boxes.npz, recorded by
tests/golden/make_golden_patch_boxes.py), batch contents equal to numpy's `pad` of the slices, the dataset's file forms and byte
budget, and `next()` through `train_step`."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

from segmamba_amd.dataloading import CaseDataset, PatchLoader
from segmamba_amd.trainer import build_training_state, train_step
from tests import preprocess_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_boxes.npz")


def _loader(probabilistic, dataset=None, **kw):
    return PatchLoader(R.patch_standin_dataset() if dataset is None else dataset, R.PATCH_SIZE, batch_size=R.PATCH_BATCH,
                       oversample_foreground_percent=0.33, probabilistic_oversampling=probabilistic, device="cpu", **kw)


def _replay(name):
    """-> (keys, forced, lbs, ubs) of PatchLoader for the scenario, drawn as the fixture was"""
    probabilistic, seed = R.PATCH_SCENARIOS[name]
    loader = _loader(probabilistic)
    asked = []
    inner = loader.get_bbox

    def recording(data_shape, force_fg, class_locations, *a, **k):
        lo, up = inner(data_shape, force_fg, class_locations, *a, **k)
        asked.append((bool(force_fg), lo, up))
        return lo, up
    loader.get_bbox = recording
    np.random.seed(seed)
    keys = [[int(k) for k in loader.next_batch()["keys"]] for _ in range(R.PATCH_BATCHES)]
    shape = (R.PATCH_BATCHES, R.PATCH_BATCH)
    return (np.asarray(keys), np.asarray([a[0] for a in asked]).reshape(shape), np.asarray([a[1] for a in asked]).reshape(shape + (3,)),
            np.asarray([a[2] for a in asked]).reshape(shape + (3,)))


@pytest.mark.parametrize("name", sorted(R.PATCH_SCENARIOS))
def test_keys_and_boxes_equal_the_reference_loader(name):
    z = np.load(GOLDEN)
    keys, forced, lbs, ubs = _replay(name)
    assert np.array_equal(keys, z[name + "_keys"])
    assert np.array_equal(forced, z[name + "_forced"].astype(bool))
    assert np.array_equal(lbs, z[name + "_lbs"]) and np.array_equal(ubs, z[name + "_ubs"])


def test_the_recorded_set_covers_the_cases_that_matter():
    """conditions on the fixture: every kind of case was drawn, forced and not; a forced-foreground box that the lower clamp moved;
    boxes with a negative lower bound for the odd and for the even need_to_pad; both oversampling rules differ in their flags"""
    z = np.load(GOLDEN)
    shapes = [it["data"].shape[1:] for it in R.patch_standin_dataset()]
    patch = np.asarray(R.PATCH_SIZE)
    seen_clamped = seen_odd = seen_even = seen_empty_forced = 0
    for name, (probabilistic, _) in R.PATCH_SCENARIOS.items():
        keys, forced, lbs, ubs = z[name + "_keys"], z[name + "_forced"].astype(bool), z[name + "_lbs"], z[name + "_ubs"]
        assert np.array_equal(ubs - lbs, np.broadcast_to(patch, lbs.shape))
        assert set(keys.reshape(-1).tolist()) == {0, 1, 2, 3, 4}
        last = np.zeros(R.PATCH_BATCH, dtype=bool)
        last[round(R.PATCH_BATCH * (1 - 0.33)):] = True
        assert probabilistic != bool(np.array_equal(forced, np.broadcast_to(last, forced.shape)))
        # case 1's foreground lies in z <= 3: a patch centred there would start at z <= 3 - 8 and is moved up to the lower bound 0
        clamped = forced & (keys == R.PATCH_CLAMP_CASE)
        assert (lbs[clamped][:, 0] == 0).all()
        seen_clamped += int(clamped.sum())
        odd, even = keys == R.PATCH_ODD_CASE, keys == R.PATCH_EVEN_CASE
        assert shapes[R.PATCH_ODD_CASE][0] == 13 and shapes[R.PATCH_EVEN_CASE][1] == 12
        assert np.isin(lbs[odd & ~forced][:, 0], (-2, -1)).all() and (lbs[even & ~forced][:, 1] == -2).all()
        seen_odd += int((lbs[odd][:, 0] < 0).sum())
        seen_even += int((lbs[even][:, 1] < 0).sum())
        seen_empty_forced += int((forced & (keys == R.PATCH_EMPTY_CASE)).sum())
    assert seen_clamped >= 1 and seen_odd >= 1 and seen_even >= 1 and seen_empty_forced >= 1


def test_batch_contents_equal_numpy_pad_of_the_slices():
    dataset = R.patch_standin_dataset()
    loader = _loader(False, dataset)
    np.random.seed(5)
    padded = 0
    for _ in range(6):
        state = np.random.get_state()
        batch = loader.next_batch()
        np.random.set_state(state)
        keys, picks = loader._draw()                       # the same draws again: the boxes of this batch
        assert np.array_equal(keys, batch["keys"]) and [p["name"] for p in batch["properties"]] == [f"case_{k}" for k in keys]
        assert batch["data"].dtype == torch.float32 and tuple(batch["data"].shape) == (R.PATCH_BATCH, 2) + R.PATCH_SIZE
        assert tuple(batch["seg"].shape) == (R.PATCH_BATCH, 1) + R.PATCH_SIZE
        for j, (key, (_, lower, upper)) in enumerate(zip(keys, picks)):
            item = dataset[key]
            shape = item["data"].shape[1:]
            sl = tuple(slice(max(0, lo), min(n, up)) for lo, up, n in zip(lower, upper, shape))
            pad = [(0, 0)] + [(-min(0, lo), max(up - n, 0)) for lo, up, n in zip(lower, upper, shape)]
            padded += int(any(p != (0, 0) for p in pad))
            for name in ("data", "seg"):
                want = np.pad(item[name][(slice(None),) + sl], pad, "constant", constant_values=0).astype(np.float32)
                assert np.array_equal(batch[name][j].numpy(), want), (name, j)
    assert padded >= 1


def test_next_maps_minus_one_to_zero_and_feeds_train_step():
    loader = _loader(False)
    np.random.seed(9)
    seen_minus = False
    for _ in range(4):
        state = np.random.get_state()
        raw = loader.next_batch()
        np.random.set_state(state)
        image, label = loader.next()
        assert torch.equal(image, raw["data"]) and label.dtype == torch.int64 and tuple(label.shape) == (R.PATCH_BATCH,) + R.PATCH_SIZE
        assert torch.equal(label, raw["seg"][:, 0].clamp(min=0).long()) and int(label.min()) == 0
        seen_minus = seen_minus or bool((raw["seg"] == -1).any())
    assert seen_minus, "the batches must have held a -1 to map"
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv3d(2, 8, 3, padding=1), nn.InstanceNorm3d(8), nn.LeakyReLU(0.01), nn.Conv3d(8, 4, 1))
    st = build_training_state(torch.device("cpu"), model=model)
    before = [p.detach().clone() for p in st.model.parameters()]
    loss = train_step(st, image, label)
    assert torch.isfinite(loss) and any((a - b.detach()).abs().max() > 0 for a, b in zip(before, st.model.parameters()))
    # with the augmenter: same shapes and dtypes, labels still classes
    aug = _loader(False, augment=True, seed=3)
    x, y = aug.next()
    assert x.shape == image.shape and y.shape == label.shape and y.dtype == torch.int64 and 0 <= int(y.min()) and int(y.max()) <= 3


def _write_cases(folder, unpacked=()):
    paths = []
    for i, item in enumerate(R.patch_standin_dataset()):
        stem = os.path.join(str(folder), item["properties"]["name"])
        np.savez_compressed(stem + ".npz", data=item["data"], seg=item["seg"])
        with open(stem + ".pkl", "wb") as f:
            pickle.dump(item["properties"], f)
        if i in unpacked:
            np.save(stem + ".npy", item["data"])
            np.save(stem + "_seg.npy", item["seg"])
        paths.append(stem + ".npz")
    return paths


def test_case_dataset_reads_both_file_forms_and_keeps_to_its_budget(tmp_path):
    paths = _write_cases(tmp_path, unpacked=(1, 3))
    want = R.patch_standin_dataset()
    ds = CaseDataset(paths, device="cpu")
    assert len(ds) == 5
    for i in range(5):
        item = ds[i]
        assert set(item) == {"data", "seg", "properties"} and item["properties"]["name"] == f"case_{i}"
        assert item["data"].dtype == torch.float32 and np.array_equal(item["data"].numpy(), want[i]["data"])
        assert item["seg"].dtype == torch.int8 and np.array_equal(item["seg"].numpy(), want[i]["seg"])
        assert ds[i]["data"] is item["data"], "a case that fits the budget is uploaded once"
    assert ds.cached_bytes == sum(w["data"].nbytes + w["seg"].nbytes for w in want)
    test = CaseDataset(paths, test=True, device="cpu")
    assert set(test[0]) == {"data", "properties"}
    with pytest.raises(RuntimeError, match="no seg"):
        PatchLoader(test, R.PATCH_SIZE, device="cpu").next_batch()
    one = want[0]["data"].nbytes + want[0]["seg"].nbytes
    small = CaseDataset(paths, device="cpu", cache_bytes=one)
    first = small[0]["data"]
    assert small[0]["data"] is first and small.cached_bytes == one
    assert small[1]["data"] is not small[1]["data"] and small.cached_bytes == one, "beyond the budget a case is uploaded per use"
    # the loader on the files draws what it draws on the stand-in
    np.random.seed(2)
    a = PatchLoader(ds, R.PATCH_SIZE, batch_size=R.PATCH_BATCH, device="cpu").next_batch()
    np.random.seed(2)
    b = _loader(False).next_batch()
    assert np.array_equal(a["keys"], b["keys"]) and torch.equal(a["data"], b["data"]) and torch.equal(a["seg"], b["seg"])
