"""Single-file NIfTI-1 reading and writing with the standard library and numpy only (host side).

The reference writes its predictions with SimpleITK (`save_to_nii`, light_training/prediction.py:208-227:
`sitk.GetImageFromArray(array)`, `SetSpacing(raw_spacing)`, `WriteImage(..., "<case>.nii.gz")`).  `write_nifti` produces the same kind
of file from a (z, y, x) array: `dim = [3, X, Y, Z, 1, 1, 1, 1]`, `pixdim[1..3]` = the spacing in the order given (the reference passes
`raw_spacing` to `SetSpacing` unpermuted, i.e. as (x, y, z) spacings), little-endian, `vox_offset` 352, magic "n+1", and
`qform_code = sform_code = 1` with ITK's LPS-to-RAS convention for an identity direction and a zero origin:
`srow_x = (-sx, 0, 0, 0)`, `srow_y = (0, -sy, 0, 0)`, `srow_z = (0, 0, sz, 0)`, quaternion (b, c, d) = (0, 0, 1), qfac 1.

That convention is taken from the format's definition (nifti1.h) and ITK's documented behaviour.  It could NOT be compared with a file
written by SimpleITK: neither SimpleITK nor nibabel is installed where this was developed, so the equality of the orientation fields
with SimpleITK's output is unverified (the voxel data, the shape and the spacing do not depend on it).

`read_nifti` reads what `write_nifti` writes and any single-file NIfTI-1 of the four supported types without extensions or scaling;
it refuses everything else with a clear error.
"""
from __future__ import annotations

import gzip
import struct
from typing import Sequence, Tuple

import numpy as np

_TYPES = {np.dtype(np.uint8): (2, 8), np.dtype(np.int16): (4, 16), np.dtype(np.int32): (8, 32), np.dtype(np.float32): (16, 32)}
_CODES = {code: dt for dt, (code, _) in _TYPES.items()}
_HDR = 348
_OFFSET = 352


def _header(shape_zyx, dtype: np.dtype, spacing: Sequence[float]) -> bytes:
    code, bits = _TYPES[dtype]
    Z, Y, X = shape_zyx
    sx, sy, sz = (float(s) for s in spacing)
    h = bytearray(_HDR)
    struct.pack_into("<i", h, 0, _HDR)                                   # sizeof_hdr
    struct.pack_into("<8h", h, 40, 3, X, Y, Z, 1, 1, 1, 1)               # dim
    struct.pack_into("<hh", h, 70, code, bits)                           # datatype, bitpix
    struct.pack_into("<8f", h, 76, 1.0, sx, sy, sz, 0.0, 0.0, 0.0, 0.0)   # pixdim (qfac = 1)
    struct.pack_into("<f", h, 108, float(_OFFSET))                       # vox_offset
    struct.pack_into("<ff", h, 112, 1.0, 0.0)                            # scl_slope, scl_inter
    h[123] = 2                                                           # xyzt_units: millimetres
    struct.pack_into("<hh", h, 252, 1, 1)                                # qform_code, sform_code
    struct.pack_into("<6f", h, 256, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)         # quatern_b, c, d, qoffset_x, y, z
    struct.pack_into("<4f", h, 280, -sx, 0.0, 0.0, 0.0)                  # srow_x
    struct.pack_into("<4f", h, 296, 0.0, -sy, 0.0, 0.0)                  # srow_y
    struct.pack_into("<4f", h, 312, 0.0, 0.0, sz, 0.0)                   # srow_z
    h[344:348] = b"n+1\0"
    return bytes(h)


def _open(path: str, mode: str):
    if path.endswith(".nii.gz"):
        return gzip.open(path, mode)
    if path.endswith(".nii"):
        return open(path, mode)
    raise RuntimeError(f"{path}: the name must end in .nii or .nii.gz")


def write_nifti(path: str, array, spacing: Sequence[float] = (1, 1, 1)) -> None:
    """array (z, y, x), as `sitk.GetImageFromArray` takes it: uint8, int16, int32 or float32 (bool is written as uint8).
    spacing: three positive numbers, written to pixdim[1..3] in the order given."""
    a = np.asarray(array)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype.newbyteorder("=") not in _TYPES:
        raise RuntimeError(f"write_nifti: uint8, int16, int32 or float32 required, got {a.dtype}")
    if a.ndim != 3 or a.size == 0:
        raise RuntimeError(f"write_nifti: a non-empty (z, y, x) array is required, got shape {a.shape}")
    if max(a.shape) > 32767:
        raise RuntimeError(f"write_nifti: NIfTI-1 limits a side to 32767 voxels, got shape {a.shape}")
    sp = tuple(float(s) for s in spacing)
    if len(sp) != 3 or not all(np.isfinite(s) and s > 0 for s in sp):
        raise RuntimeError(f"write_nifti: spacing must be three positive numbers, got {spacing}")
    dt = a.dtype.newbyteorder("=")
    data = np.ascontiguousarray(a, dtype=dt.newbyteorder("<"))
    with _open(str(path), "wb") as f:
        f.write(_header(a.shape, dt, sp))
        f.write(b"\0\0\0\0")                                             # no extensions; the data start at byte 352
        f.write(data.tobytes())


def read_nifti(path: str) -> Tuple[np.ndarray, Tuple[float, float, float]]:
    """-> (array (z, y, x), spacing = pixdim[1..3])"""
    path = str(path)
    with _open(path, "rb") as f:
        raw = f.read()
    if len(raw) < _OFFSET:
        raise RuntimeError(f"{path}: shorter than a NIfTI-1 header")
    if struct.unpack_from("<i", raw, 0)[0] != _HDR:
        if struct.unpack_from(">i", raw, 0)[0] == _HDR:
            raise RuntimeError(f"{path}: big-endian NIfTI files are not supported")
        raise RuntimeError(f"{path}: not a NIfTI-1 file (sizeof_hdr is not 348)")
    magic = raw[344:348]
    if magic != b"n+1\0":
        raise RuntimeError(f"{path}: only single-file NIfTI-1 (magic 'n+1') is supported, got {magic!r}")
    dim = struct.unpack_from("<8h", raw, 40)
    if not 1 <= dim[0] <= 7 or any(d < 1 for d in dim[1:dim[0] + 1]) or any(d > 1 for d in dim[4:dim[0] + 1]) or dim[0] < 3:
        raise RuntimeError(f"{path}: a 3-D volume is required, got dim {dim}")
    code, bits = struct.unpack_from("<hh", raw, 70)
    if code not in _CODES or _TYPES[_CODES[code]][1] != bits:
        raise RuntimeError(f"{path}: datatype {code} / bitpix {bits} is not supported (uint8, int16, int32, float32)")
    pixdim = struct.unpack_from("<8f", raw, 76)
    offset = struct.unpack_from("<f", raw, 108)[0]
    slope, inter = struct.unpack_from("<ff", raw, 112)
    if not (slope == 0.0 or (slope == 1.0 and inter == 0.0)):
        raise RuntimeError(f"{path}: scaled data (scl_slope {slope}, scl_inter {inter}) are not supported")
    if raw[348:352] != b"\0\0\0\0" and raw[348] != 0:
        raise RuntimeError(f"{path}: header extensions are not supported")
    if offset != int(offset) or int(offset) < _OFFSET:
        raise RuntimeError(f"{path}: vox_offset {offset} is not supported")
    X, Y, Z = dim[1:4]
    dt = _CODES[code]
    n = X * Y * Z
    start = int(offset)
    if len(raw) < start + n * dt.itemsize:
        raise RuntimeError(f"{path}: the file ends before its {n} voxels do")
    a = np.frombuffer(raw, dtype=dt.newbyteorder("<"), count=n, offset=start).reshape(Z, Y, X).astype(dt)
    return a, (float(pixdim[1]), float(pixdim[2]), float(pixdim[3]))
