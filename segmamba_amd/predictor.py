"""Sliding-window inference with mirror test-time augmentation: the caller of `SegMamba.forward` at prediction time
(SURVEY.md §8f rank 2).

Host-side mirror of the reference's prediction path:
  `Predictor`                light_training/prediction.py:29-227 (`maybe_mirror_and_predict`, `predict_raw_probability`,
                             `predict_noncrop_probability`, `save_to_nii`; `predict_labels` = the middle two and the arg-max
                             between them as one launch on the device, segmamba_amd/postprocess.py)
  `SlidingWindowInferer`     monai/inferers/inferer.py (the class 4_predict.py:55-59 and 3_train.py:35-37 construct), i.e.
  `sliding_window_inference` monai/inferers/utils.py:43-330 with its helpers `dense_patch_slices`
                             (monai/data/utils.py:171-211) and `compute_importance_map` (:1088-1138)
with the arguments the reference uses (roi 128^3, overlap 0.5, gaussian blending, sw_batch_size 1-2, 8-way mirroring).

What differs is where the data lives.  The reference moves every window batch result - and every one of the 8 mirrored
full-volume predictions - to host memory and accumulates there (prediction.py:126-152 `.cpu()` after each pass).  A
BraTS volume (4 x 240 x 240 x 155 fp32 = 143 MB, 4-class logits the same again) is nothing against 288 GB of HBM: here the
volume, the weighted accumulator, the weight map and the mirrored copies stay on the device for the whole prediction, the
eight mirror passes accumulate into one fp32 buffer, and windows go through the network in as large a batch as asked.

Two routes stitch the windows.  `stitch="aten"` (the default) is the chain of ATen calls below.  `stitch="hip"` runs the same
arithmetic on the kernels of csrc/stitch.hip (`_HipStitch`): the mirror and the centring padding are folded into the window gather
and into the close of a pass, the count map is built once per prediction, and a window batch is blended in one launch.  The two
routes are bit-equal; the kernel route is opt-in and never falls back.
"""
from __future__ import annotations

import itertools
import math
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


def _tuple3(v, n: int) -> Tuple:
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


def dense_patch_starts(image_size: Sequence[int], roi_size: Sequence[int], scan_interval: Sequence[int]) -> List[Tuple[int, ...]]:
    """Window origins in the reference's order (last dimension fastest; monai/data/utils.py:191-208): along every dimension
    windows start every `scan_interval`, the last one pulled back so that it ends at the image border."""
    starts = []
    for size, roi, step in zip(image_size, roi_size, scan_interval):
        if step == 0:
            num = 1
        else:
            cand = next((d for d in range(int(math.ceil(size / step))) if d * step + roi >= size), None)
            num = cand + 1 if cand is not None else 1
        starts.append([min(i * step, size - roi) for i in range(num)])
    return list(itertools.product(*starts))


def _window_weights(roi_size: Sequence[int], mode: str, sigma_scale, device) -> torch.Tensor:
    """the window weights before the clamp: ones, or the separable gaussian, fp32"""
    if mode == "constant":
        w = torch.ones(tuple(roi_size), device=device, dtype=torch.float32)
    elif mode == "gaussian":
        sig = _tuple3(sigma_scale, len(roi_size))
        w = None
        for i, n in enumerate(roi_size):
            x = torch.arange(-(n - 1) / 2.0, (n - 1) / 2.0 + 1, dtype=torch.float32, device=device)
            g = torch.exp(x ** 2 / (-2 * (n * sig[i]) ** 2))
            w = g if w is None else w.unsqueeze(-1) * g[(None,) * i]
    else:
        raise ValueError(f"Unsupported mode: {mode}, available options are ['constant', 'gaussian'].")
    return w


def importance_map(roi_size: Sequence[int], mode: str = "constant", sigma_scale=0.125, device="cpu",
                   dtype=torch.float32) -> torch.Tensor:
    """Window weights (monai/data/utils.py:1117-1138): ones, or a separable gaussian with sigma = sigma_scale * size,
    clamped from below by max(min, 1e-3)."""
    w = _window_weights(roi_size, mode, sigma_scale, device)
    return torch.clamp(w, min=max(float(w.min()), 1e-3)).to(dtype)


def _importance_map_no_sync(roi_size: Sequence[int], mode: str, sigma_scale, device) -> torch.Tensor:
    """`importance_map` in fp32 with the clamp's bound kept on the device: the same bits (the bound is max(min, fl32(1e-3)) either
    way, no fp32 value lies between 1e-3 and its fp32 rounding), and nothing is read back to the host"""
    w = _window_weights(roi_size, mode, sigma_scale, device)
    return torch.clamp(w, min=torch.clamp(w.min(), min=1e-3))


STITCH_ROUTES = ("aten", "hip")


def _check_stitch(stitch) -> str:
    if stitch not in STITCH_ROUTES:
        raise ValueError(f"Unsupported stitch: {stitch!r}, available options are {list(STITCH_ROUTES)}.")
    return stitch


class _HipStitch:
    """One prediction on the kernels of csrc/stitch.hip: the geometry of `sliding_window_inference`, the weight map and the count
    map (once), then per mirror pass `run_pass`: gather a window batch, run the predictor, blend; one finish closes the pass.  The
    accumulator and the total are shared by the passes.  Nothing is copied to the host and nothing waits for the device."""

    def __init__(self, inputs: torch.Tensor, roi_size, sw_batch_size: int, overlap, mode: str, sigma_scale, padding_mode: str,
                 cval: float) -> None:
        from . import lib as L
        if not isinstance(inputs, torch.Tensor) or inputs.dim() != 5:
            raise NotImplementedError(f'stitch="hip" takes 3-D volumes (B, C, Z, Y, X), got shape {tuple(getattr(inputs, "shape", ()))}; '
                                      'use stitch="aten"')
        if inputs.dtype != torch.float32:
            raise NotImplementedError(f'stitch="hip" takes float32 volumes, got {inputs.dtype}; use stitch="aten"')
        if padding_mode != "constant":
            raise NotImplementedError(f'stitch="hip" pads with a constant only, got padding_mode={padding_mode!r}; use stitch="aten"')
        if not L.on_device(inputs):
            raise RuntimeError(f'stitch="hip" runs on the HIP library\'s kernels (csrc/stitch.hip): the volume must live on the GPU, '
                               f'got a tensor on {inputs.device}; use stitch="aten" on host tensors')
        if int(sw_batch_size) < 1:
            raise ValueError(f"sw_batch_size must be at least 1, got {sw_batch_size}.")
        self.lib = L.get_lib()
        overlap = _tuple3(overlap, 3)
        if any(o < 0 or o >= 1 for o in overlap):
            raise ValueError(f"overlap must be >= 0 and < 1, got {overlap}.")
        self.batch = int(inputs.shape[0])
        self.size = tuple(int(v) for v in inputs.shape[2:])
        self.roi = tuple(int(r) if r and r > 0 else int(s) for r, s in zip(_tuple3(roi_size, 3), self.size))
        self.image = tuple(max(s, r) for s, r in zip(self.size, self.roi))
        interval = tuple(r if r == s else max(int(r * (1 - o)), 1) for r, s, o in zip(self.roi, self.image, overlap))
        starts = dense_patch_starts(self.image, self.roi, interval)
        self.jobs = [(b,) + tuple(st) for b in range(self.batch) for st in starts]
        self.sw_batch_size, self.cval = int(sw_batch_size), float(cval)
        from . import ops_raw
        self.ops = ops_raw
        self.weight = _importance_map_no_sync(self.roi, mode, sigma_scale, inputs.device)
        axis_starts = [sorted(set(st[d] for st in starts)) for d in range(3)]
        self.count = ops_raw.window_count(self.lib, self.weight, self.size, axis_starts)
        self.acc: Optional[torch.Tensor] = None

    def run_pass(self, x: torch.Tensor, predictor: Callable[..., torch.Tensor], mirror: int, total: Optional[torch.Tensor],
                 index: int, passes: int, *args, **kwargs) -> torch.Tensor:
        """mirror pass `index` of `passes` of the volume x under the flip mask `mirror` -> total (allocated on pass 0)"""
        from . import lib as L
        if tuple(x.shape[2:]) != self.size or int(x.shape[0]) != self.batch or x.dtype != torch.float32 or not L.on_device(x):
            raise RuntimeError(f'stitch="hip": the volume changed between passes: {tuple(x.shape)} {x.dtype} on {x.device}')
        lib, ops, cap = self.lib, self.ops, L.STITCH_MAX_WINDOWS
        for j0 in range(0, len(self.jobs), self.sw_batch_size):
            chunk = self.jobs[j0:j0 + self.sw_batch_size]
            parts = [ops.window_gather(lib, x, self.roi, chunk[k:k + cap], mirror, self.cval) for k in range(0, len(chunk), cap)]
            win = parts[0] if len(parts) == 1 else torch.cat(parts)
            pred = predictor(win, *args, **kwargs)
            if not isinstance(pred, torch.Tensor) or pred.dim() != 5 or tuple(pred.shape[2:]) != self.roi:
                raise RuntimeError("sliding_window_inference: the predictor must keep the window's spatial size")
            if int(pred.shape[0]) != len(chunk):
                raise RuntimeError(f"sliding_window_inference: the predictor returned {int(pred.shape[0])} windows for {len(chunk)}")
            if not L.on_device(pred) or pred.device != x.device:
                raise RuntimeError(f'stitch="hip": the predictor\'s output must stay on {x.device}, got {pred.device}')
            if pred.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                raise NotImplementedError(f'stitch="hip" blends float32, bfloat16 or float16 predictions, got {pred.dtype}')
            if self.acc is None:
                self.acc = torch.zeros((self.batch, int(pred.shape[1])) + self.image, dtype=torch.float32, device=x.device)
            elif int(pred.shape[1]) != int(self.acc.shape[1]):
                raise RuntimeError(f"sliding_window_inference: the predictor returned {int(pred.shape[1])} channels after "
                                   f"{int(self.acc.shape[1])}")
            pred = pred.detach().contiguous()
            for k in range(0, len(chunk), cap):
                ops.window_blend(lib, self.acc, pred[k:k + cap], self.weight, chunk[k:k + cap])
        if total is None:
            total = torch.empty(tuple(self.acc.shape[:2]) + self.size, dtype=torch.float32, device=x.device)
        return ops.window_finish(lib, self.acc, self.count, total, self.roi, mirror, index, passes)


def sliding_window_inference(inputs: torch.Tensor, roi_size, sw_batch_size: int, predictor: Callable[..., torch.Tensor],
                             overlap=0.25, mode: str = "constant", sigma_scale=0.125, padding_mode: str = "constant",
                             cval: float = 0.0, *args, stitch: str = "aten", **kwargs) -> torch.Tensor:
    """inputs (B, C, *spatial) -> predictor outputs stitched to (B, C_out, *spatial); the reference's blending:
    sum_w (weight * prediction) / sum_w weight, accumulated in the input's dtype on the input's device.
    `stitch="hip"` (keyword only): the same result, bit for bit, on the kernels of csrc/stitch.hip - 3-D float32 volumes on the
    GPU with constant padding; anything else raises."""
    if _check_stitch(stitch) == "hip":
        return _HipStitch(inputs, roi_size, sw_batch_size, overlap, mode, sigma_scale, padding_mode, cval).run_pass(
            inputs, predictor, 0, None, 0, 1, *args, **kwargs)
    nd = inputs.dim() - 2
    overlap = _tuple3(overlap, nd)
    if any(o < 0 or o >= 1 for o in overlap):
        raise ValueError(f"overlap must be >= 0 and < 1, got {overlap}.")
    batch, _, *orig_size = inputs.shape
    roi = tuple(int(r) if r and r > 0 else int(s) for r, s in zip(_tuple3(roi_size, nd), orig_size))
    image_size = tuple(max(s, r) for s, r in zip(orig_size, roi))
    pad = []
    for k in range(nd - 1, -1, -1):                        # images smaller than the window are centred in padding
        diff = max(roi[k] - orig_size[k], 0)
        pad.extend([diff // 2, diff - diff // 2])
    if any(pad):
        inputs = F.pad(inputs, pad, mode=padding_mode, value=cval)
    interval = tuple(r if r == s else max(int(r * (1 - o)), 1) for r, s, o in zip(roi, image_size, overlap))
    starts = dense_patch_starts(image_size, roi, interval)
    weight = importance_map(roi, mode, sigma_scale, inputs.device, inputs.dtype)[None, None]

    out: Optional[torch.Tensor] = None
    count = torch.zeros((1, 1) + image_size, dtype=inputs.dtype, device=inputs.device)
    for st in starts:
        count[(slice(None), slice(None)) + tuple(slice(s, s + r) for s, r in zip(st, roi))] += weight
    jobs = [(b, st) for b in range(batch) for st in starts]
    for j0 in range(0, len(jobs), sw_batch_size):
        chunk = jobs[j0:j0 + sw_batch_size]
        win = torch.cat([inputs[(slice(b, b + 1), slice(None)) + tuple(slice(s, s + r) for s, r in zip(st, roi))]
                         for b, st in chunk])
        pred = predictor(win, *args, **kwargs)
        if pred.shape[2:] != roi:
            raise RuntimeError("sliding_window_inference: the predictor must keep the window's spatial size")
        if out is None:
            out = torch.zeros((batch, pred.shape[1]) + image_size, dtype=inputs.dtype, device=inputs.device)
        pred = pred.to(inputs.dtype) * weight
        for i, (b, st) in enumerate(chunk):
            out[(slice(b, b + 1), slice(None)) + tuple(slice(s, s + r) for s, r in zip(st, roi))] += pred[i:i + 1]
    out = out / count
    if any(pad):                                            # remove the centring padding again
        sl = [slice(None), slice(None)]
        for d in range(nd):
            p0 = pad[2 * (nd - 1 - d)]
            sl.append(slice(p0, p0 + orig_size[d]))
        out = out[tuple(sl)]
    return out


class SlidingWindowInferer:
    """Constructor-compatible with the object the reference builds (4_predict.py:55-59, 3_train.py:35-37)."""

    def __init__(self, roi_size, sw_batch_size: int = 1, overlap=0.25, mode: str = "constant", sigma_scale=0.125,
                 padding_mode: str = "constant", cval: float = 0.0, progress: bool = False, stitch: str = "aten", **unused) -> None:
        self.roi_size, self.sw_batch_size, self.overlap = roi_size, sw_batch_size, overlap
        self.mode, self.sigma_scale, self.padding_mode, self.cval = mode, sigma_scale, padding_mode, cval
        self.stitch = _check_stitch(stitch)

    def __call__(self, inputs: torch.Tensor, network: Callable[..., torch.Tensor], *args, **kwargs) -> torch.Tensor:
        return sliding_window_inference(inputs, self.roi_size, self.sw_batch_size, network, self.overlap, self.mode,
                                        self.sigma_scale, self.padding_mode, self.cval, *args, stitch=self.stitch, **kwargs)

    def stitcher(self, inputs: torch.Tensor) -> _HipStitch:
        """the kernel route's state for one prediction of `inputs` (stitch="hip")"""
        return _HipStitch(inputs, self.roi_size, self.sw_batch_size, self.overlap, self.mode, self.sigma_scale, self.padding_mode,
                          self.cval)


class Predictor:
    """reference light_training/prediction.py:29-159, device-resident."""

    def __init__(self, window_infer, mirror_axes=None, autocast_dtype: torch.dtype = torch.bfloat16) -> None:
        """`autocast_dtype`: the reference runs the network under `torch.autocast("cuda")`, i.e. fp16 (prediction.py:124);
        on MI355X the path's 16-bit type is bf16 (BASELINE north star), so that is the default.  Pass torch.float16 for
        the reference's behaviour (same kernels, same speed)."""
        self.window_infer = window_infer
        self.mirror_axes = mirror_axes
        self.autocast_dtype = autocast_dtype

    def maybe_mirror_and_predict(self, x: torch.Tensor, model, device=torch.device("cpu"), **kwargs) -> torch.Tensor:
        """Mean over the 2^len(mirror_axes) mirrored sliding-window predictions (reference :110-159).  The sum runs in the
        reference's order (identity, each single axis, each pair, all three) in fp32 on `device`; the result stays there."""
        device = torch.device(device) if isinstance(device, str) else device
        model.to(device)
        x = x.to(device)
        axes = self.mirror_axes
        if axes is not None and len(axes) and max(axes) > x.dim() - 3:
            raise AssertionError("mirror_axes does not match the dimension of the input!")
        combos: List[Tuple[int, ...]] = [()]
        if axes is not None:
            ordered = sorted(axes)
            for k in range(1, len(ordered) + 1):
                combos += list(itertools.combinations(ordered, k))
        with torch.no_grad(), torch.autocast("cuda", dtype=self.autocast_dtype,
                                             enabled=device.type == "cuda" and self.autocast_dtype != torch.float32):
            total = None
            if isinstance(self.window_infer, SlidingWindowInferer) and self.window_infer.stitch == "hip":
                # one accumulator, one count map and one total for all passes; the mirror is an index in gather and finish
                state = self.window_infer.stitcher(x)
                for i, c in enumerate(combos):
                    total = state.run_pass(x, model, sum(1 << a for a in c), total, i, len(combos), **kwargs)
                return total
            for c in combos:
                dims = tuple(a + 2 for a in c)
                xin = torch.flip(x, dims) if dims else x
                p = self.window_infer(xin, model, **kwargs).float()
                p = torch.flip(p, dims) if dims else p
                total = p if total is None else total + p
            return total / len(combos)

    @staticmethod
    def predict_raw_probability(model_output: torch.Tensor, properties: dict) -> torch.Tensor:
        """trilinear resampling back to the pre-resample crop shape, channel by channel (reference :33-62)."""
        if model_output.dim() == 5:
            model_output = model_output[0]
        d, w, h = (int(v) for v in properties["shape_after_cropping_before_resample"][:3])
        with torch.no_grad():
            return torch.stack([F.interpolate(model_output[c][None, None].float(), size=(d, w, h), mode="trilinear")[0, 0]
                                for c in range(model_output.shape[0])]).to(model_output.dtype)

    @staticmethod
    def predict_noncrop_probability(model_output, properties: dict) -> np.ndarray:
        """paste the cropped prediction back into the full-size uint8 volume (reference :64-108)."""
        if isinstance(model_output, torch.Tensor):
            model_output = model_output.cpu().numpy()
        shape = [int(v.item()) if isinstance(v, torch.Tensor) else int(v) for v in properties["shape_before_cropping"][:3]]
        (a0, a1), (b0, b1), (c0, c1) = [tuple(int(v) for v in bb) for bb in properties["bbox_used_for_cropping"][:3]]
        if model_output.ndim == 3:
            full = np.zeros(shape, dtype=np.uint8)
            full[a0:a1, b0:b1, c0:c1] = model_output
        elif model_output.ndim == 4:
            full = np.zeros([model_output.shape[0]] + shape, dtype=np.uint8)
            full[:, a0:a1, b0:b1, c0:c1] = model_output
        else:
            raise ValueError("restore crop error: expected a 3-D label map or a 4-D (C, ...) volume")
        return full

    @staticmethod
    def predict_labels(model_output, properties: Optional[dict] = None) -> torch.Tensor:
        """`predict_raw_probability` -> `argmax` over the classes -> `predict_noncrop_probability` (4_predict.py:78-83) in one launch on
        the device: the uint8 label volume of `shape_before_cropping` (segmamba_amd.postprocess.labels_from_logits).  The resampled
        logits are compared in fp32, as the reference's CPU branch does."""
        from . import postprocess
        return postprocess.labels_from_logits(model_output, properties)

    def save_to_nii(self, return_output, raw_spacing, save_dir, case_name, postprocess: bool = False, connectivity: int = 1) -> str:
        """Write `<save_dir>/<case_name>.nii.gz` (reference :208-227).  `return_output`: a (D, H, W) label volume or mask, device tensor,
        host tensor or numpy array; it is cast to uint8 as the reference does.  `postprocess` runs `largest_connected_domain` on the
        device (an empty mask stays empty where the reference raises) with components at `connectivity` (1, 2, 3; the reference's 1 by
        default; the holes are filled at background connectivity 1).  `raw_spacing` goes to the header unpermuted, as the reference
        passes it to `SetSpacing`.
        A (C, D, H, W) input is refused unless C == 1: SimpleITK would turn a 4-D array into a 3-D VECTOR image, which nothing
        downstream of the reference reads as labels (4_predict.py passing its (3, ...) region stack is the reference's own loose end);
        write one file per channel instead.  -> the path written."""
        import os

        from . import nifti
        from . import ops_raw
        from . import postprocess as post
        connectivity = ops_raw._connectivity(connectivity, "save_to_nii")
        out = return_output
        shape = tuple(out.shape)
        if len(shape) == 4 and shape[0] == 1:
            out = out[0]
        elif len(shape) != 3:
            raise RuntimeError(f"save_to_nii: a (D, H, W) volume (or (1, D, H, W)) is required, got shape {shape}; a (C, D, H, W) stack "
                               "would become a vector image in the reference - write one file per channel")
        if postprocess:
            out = post.largest_connected_domain(out, connectivity=connectivity)    # uploads numpy / host tensors, stays on the device
        if isinstance(out, torch.Tensor):
            out = out.to(torch.uint8).cpu().numpy()                        # the one copy to the host: one byte per voxel
        else:
            out = np.asarray(out).astype(np.uint8)
        spacing = [float(v.item()) if isinstance(v, torch.Tensor) else float(v) for v in list(raw_spacing)[:3]]
        os.makedirs(save_dir, exist_ok=True)
        path = os.path.join(save_dir, f"{case_name}.nii.gz")
        nifti.write_nifti(path, out, spacing)
        print(f"{path} is saved successfully")
        return path

    def save_organs_to_nii(self, labels, raw_spacing, save_dir, names: Sequence[str], postprocess: bool = False,
                           connectivity: int = 1) -> List[str]:
        """One file per organ of a multi-class label map: `<save_dir>/<names[i - 1]>.nii.gz` holds `labels == i` for i = 1 .. len(names)
        (the loop of the reference's light_training/examples/AbdomenAtlas1.0Mini/4_predict_diffunet.py:97-109).  `labels`: a (D, H, W)
        label volume, device tensor, host tensor or numpy array.  With `postprocess` each organ is `binary_fill_holes` of its largest
        component (`large_connected_domain` per organ); the largest components of all organs come from ONE labelled pass on the device
        (segmamba_amd.postprocess.keep_largest_per_class) with components at `connectivity` (1, 2, 3; holes at background connectivity
        1).  One copy to the host: the uint8 label volume, or with `postprocess` the
        organs' filled masks packed eight to a byte (filled holes of different organs may overlap).  -> the paths written."""
        import os

        from . import nifti
        from . import ops_raw
        from . import postprocess as post
        connectivity = ops_raw._connectivity(connectivity, "save_organs_to_nii")
        names = [str(n) for n in names]
        if not 1 <= len(names) <= 255 or len(set(names)) != len(names):
            raise RuntimeError(f"save_organs_to_nii: between 1 and 255 distinct organ names are required, got {names}")
        shape = tuple(labels.shape)
        if len(shape) == 4 and shape[0] == 1:
            labels = labels[0]
        elif len(shape) != 3:
            raise RuntimeError(f"save_organs_to_nii: a (D, H, W) label volume (or (1, D, H, W)) is required, got shape {shape}")
        n = len(names)
        if postprocess:
            kept = post.keep_largest_per_class(labels, classes=range(1, n + 1), connectivity=connectivity)
            packed = torch.zeros(((n + 7) // 8,) + tuple(kept.shape), dtype=torch.uint8, device=kept.device)
            for i in range(n):
                packed[i // 8] |= post.binary_fill_holes(kept == i + 1) << (i % 8)
            host = packed.cpu().numpy()                                   # the one copy to the host
            organs = [((host[i // 8] >> (i % 8)) & 1).astype(np.uint8) for i in range(n)]
        else:
            host = labels.to(torch.uint8).cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels).astype(np.uint8)
            organs = [(host == i + 1).astype(np.uint8) for i in range(n)]
        spacing = [float(v.item()) if isinstance(v, torch.Tensor) else float(v) for v in list(raw_spacing)[:3]]
        os.makedirs(save_dir, exist_ok=True)
        paths = []
        for name, organ in zip(names, organs):
            paths.append(os.path.join(save_dir, f"{name}.nii.gz"))
            nifti.write_nifti(paths[-1], organ, spacing)
        print(f"{len(paths)} organ files are saved to {save_dir}")
        return paths
