"""Image file I/O for the drivers (validate / predict_cases): what the reference does through SimpleITK
(preprocessing/cropping.py:61-81 `load_case_from_list_of_files`, inference/segmentation_export.py:148-160).

SimpleITK is used when it is importable.  Otherwise `.nii` / `.nii.gz` files are read and written by the small NIfTI-1
codec below (single-file format, little endian, scalar volumes, sform or qform geometry): enough for CT volumes and label
maps, nothing else.  Geometry follows ITK's conventions so that the `itk_*` properties of a case mean the same thing either
way: arrays are indexed [z, y, x], spacing / origin are (x, y, z), the direction is the row-major 3x3 cosine matrix in LPS
(NIfTI stores RAS: x and y are negated on the way in and out).  Host code, with one exception: a uint8 label map that is already
on the device and goes to a `.nii.gz` is gzip-encoded there (`write_label_map_device`), behind the same header, and
`read_image_device` inflates a `.nii.gz` on the device."""
import gzip
import struct

import numpy as np

_DTYPES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16, 768: np.uint32,
           1024: np.int64, 1280: np.uint64}
_CODES = {np.dtype(v).name: k for k, v in _DTYPES.items()}
_LPS = np.diag([-1.0, -1.0, 1.0])


def _have_sitk():
    try:
        import SimpleITK  # noqa: F401
        return True
    except ImportError:
        return False


class Image(object):
    """array [z, y, x] + ITK-style geometry."""

    def __init__(self, array, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
        self.array = array
        self.spacing = tuple(float(i) for i in spacing)
        self.origin = tuple(float(i) for i in origin)
        self.direction = tuple(float(i) for i in direction)

    def GetSize(self):
        return tuple(int(i) for i in self.array.shape[::-1])

    def GetSpacing(self):
        return self.spacing

    def GetOrigin(self):
        return self.origin

    def GetDirection(self):
        return self.direction


def _quaternion_to_matrix(b, c, d, qfac):
    a2 = 1.0 - (b * b + c * c + d * d)
    a = np.sqrt(a2) if a2 > 1e-7 else 0.0
    if a == 0.0:
        n = 1.0 / np.sqrt(b * b + c * c + d * d)
        b, c, d = b * n, c * n, d * n
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])
    if qfac < 0:
        R[:, 2] = -R[:, 2]
    return R


def _matrix_to_quaternion(R):
    """-> (b, c, d, qfac) of a 3x3 orthonormal matrix (nifti1_io's mat44_to_quatern without the polar decomposition)."""
    R = np.array(R, dtype=np.float64)
    qfac = 1.0
    if np.linalg.det(R) < 0:
        R[:, 2] = -R[:, 2]
        qfac = -1.0
    a = R[0, 0] + R[1, 1] + R[2, 2] + 1.0
    if a > 0.5:
        a = 0.5 * np.sqrt(a)
        b, c, d = 0.25 * (R[2, 1] - R[1, 2]) / a, 0.25 * (R[0, 2] - R[2, 0]) / a, 0.25 * (R[1, 0] - R[0, 1]) / a
    else:
        xd, yd, zd = 1.0 + R[0, 0] - (R[1, 1] + R[2, 2]), 1.0 + R[1, 1] - (R[0, 0] + R[2, 2]), 1.0 + R[2, 2] - (R[0, 0] + R[1, 1])
        if xd > 1.0:
            b = 0.5 * np.sqrt(xd)
            c, d, a = 0.25 * (R[0, 1] + R[1, 0]) / b, 0.25 * (R[0, 2] + R[2, 0]) / b, 0.25 * (R[2, 1] - R[1, 2]) / b
        elif yd > 1.0:
            c = 0.5 * np.sqrt(yd)
            b, d, a = 0.25 * (R[0, 1] + R[1, 0]) / c, 0.25 * (R[1, 2] + R[2, 1]) / c, 0.25 * (R[0, 2] - R[2, 0]) / c
        else:
            d = 0.5 * np.sqrt(zd)
            b, c, a = 0.25 * (R[0, 2] + R[2, 0]) / d, 0.25 * (R[1, 2] + R[2, 1]) / d, 0.25 * (R[1, 0] - R[0, 1]) / d
        if a < 0:
            b, c, d = -b, -c, -d
    return float(b), float(c), float(d), qfac


def _parse_nifti(raw, fname):
    """raw: at least the 348 header bytes of a single-file NIfTI-1 -> (dtype with the file's byte order, (nz, ny, nx), voxel offset,
    slope, intercept, spacing, origin, direction), geometry in ITK's conventions"""
    if len(raw) < 348:
        raise IOError("%s: not a NIfTI-1 file (shorter than its header)" % fname)
    end = '<'
    if struct.unpack('<i', raw[:4])[0] != 348:
        end = '>'
        if struct.unpack('>i', raw[:4])[0] != 348:
            raise IOError("%s: not a NIfTI-1 file (sizeof_hdr != 348)" % fname)
    if raw[344:347] != b'n+1':
        raise IOError("%s: only single-file NIfTI-1 ('n+1') is supported" % fname)
    dim = struct.unpack(end + '8h', raw[40:56])
    datatype, = struct.unpack(end + 'h', raw[70:72])
    pixdim = struct.unpack(end + '8f', raw[76:108])
    vox_offset, slope, inter = struct.unpack(end + '3f', raw[108:120])
    qform_code, sform_code = struct.unpack(end + '2h', raw[252:256])
    if datatype not in _DTYPES:
        raise IOError("%s: unsupported NIfTI datatype code %d" % (fname, datatype))
    nd = dim[0]
    if nd < 3 or any(d != 1 for d in dim[4:nd + 1]):
        raise IOError("%s: only 3D scalar volumes are supported (dim = %s)" % (fname, str(dim)))
    nx, ny, nz = dim[1:4]
    dt = np.dtype(_DTYPES[datatype]).newbyteorder(end)
    # geometry precedence as ITK's NiftiImageIO (the reference reads through SimpleITK): the qform (rotation from the quaternion, spacing
    # from pixdim) when qform_code > 0, else the sform (spacing = column norms); a file whose two transforms disagree then gives the
    # same spacing / direction whether or not SimpleITK is installed
    if qform_code > 0:
        b, c, d, qx, qy, qz = struct.unpack(end + '6f', raw[256:280])
        Rras = _quaternion_to_matrix(b, c, d, -1.0 if pixdim[0] < 0 else 1.0)
        spacing, t = np.abs(np.array(pixdim[1:4], dtype=np.float64)), np.array([qx, qy, qz], dtype=np.float64)
    elif sform_code > 0:
        A = np.array([struct.unpack(end + '4f', raw[280 + 16 * r:296 + 16 * r]) for r in range(3)], dtype=np.float64)
        M, t = A[:, :3], A[:, 3]
        spacing = np.sqrt((M * M).sum(0))
        Rras = M / spacing
    else:
        Rras, spacing, t = np.diag([-1.0, -1.0, 1.0]), np.abs(np.array(pixdim[1:4], dtype=np.float64)), np.zeros(3)
    return dt, (nz, ny, nx), int(vox_offset), slope, inter, spacing, _LPS @ t, (_LPS @ Rras).ravel()


def _is_scaled(slope, inter):
    return bool(slope != 0 and not (slope == 1 and inter == 0) and np.isfinite(slope))


def _read_nifti(fname):
    opener = gzip.open if fname.endswith('.gz') else open
    with opener(fname, 'rb') as f:
        raw = f.read()
    dt, (nz, ny, nx), off, slope, inter, spacing, origin, direction = _parse_nifti(raw, fname)
    arr = np.frombuffer(raw, dtype=dt, count=nx * ny * nz, offset=off).reshape(nz, ny, nx)
    arr = arr.astype(dt.newbyteorder('='))
    if _is_scaled(slope, inter):
        arr = arr.astype(np.float64) * slope + inter
    return Image(arr, spacing, origin, direction)


def gzip_payload(blob, fname=''):
    """blob: one gzip member -> (offset and length of its raw DEFLATE stream, CRC-32, ISIZE).  FEXTRA, FNAME, FCOMMENT and FHCRC
    are honoured (RFC 1952)."""
    if len(blob) < 18 or blob[:2] != b'\x1f\x8b' or blob[2] != 8:
        raise IOError("%s: not a gzip member with a DEFLATE stream" % fname)
    flags, p = blob[3], 10
    try:
        if flags & 4:
            p += 2 + struct.unpack('<H', blob[p:p + 2])[0]
        for bit in (8, 16):
            if flags & bit:
                p = blob.index(b'\0', p) + 1
    except (ValueError, struct.error):
        raise IOError("%s: the gzip header is cut short" % fname)
    if flags & 2:
        p += 2
    if p + 8 >= len(blob):
        raise IOError("%s: the gzip header is cut short" % fname)
    crc, isize = struct.unpack('<II', blob[-8:])
    return p, len(blob) - 8 - p, crc, isize


def read_image_device(fname, device, stages=None):
    """A `.nii.gz` volume read onto the device: the file's compressed bytes are uploaded and inflated there (ops.inflate_raw,
    DESIGN §6y), CRC-32 and ISIZE of the gzip trailer are checked, the header comes back and is parsed by `_parse_nifti`, and the
    voxels are a view behind it -> (device tensor [z, y, x], spacing, origin, direction).  A stream without restart points or one
    the unit rules refuse (a file of another writer; a damaged one is then refused by zlib), a non-native byte order or a slope /
    intercept takes the host path: `read_image` and an upload — unless the file holds at least ops.INFLATE_SPEC_MIN_OUT bytes and
    ops.inflate_stream decodes it from block starts it finds in the stream.  A trailer that differs after a successful
    decode is an IOError.  stages['path'] says 'device' or 'host' and stages['route'] 'restart' or 'speculative'; the seconds of
    'file', 'upload', 'scan', 'write' (or 'search', 'size', 'chain', 'symbols', 'windows', 'resolve') and 'crc' are added."""
    import time
    import torch
    from .. import ops
    fname = str(fname)
    t0 = time.perf_counter()
    with open(fname, 'rb') as f:
        blob = f.read()
    p, n, crc, isize = gzip_payload(blob, fname)
    t1 = time.perf_counter()
    comp = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8, count=n, offset=p).copy()).to(device)
    if stages is not None:
        torch.cuda.synchronize(comp.device)
        stages['file'] = stages.get('file', 0.0) + (t1 - t0)
        stages['upload'] = stages.get('upload', 0.0) + (time.perf_counter() - t1)
    route = 'restart'
    try:
        out, got, _ = ops.inflate_raw(comp, stages=stages)
    except (ops.InflateForeign, IOError):
        # no restart points, or a stream the unit rules refuse (BAD / CORRUPT: a valid sync-flushed stream of zlib or pigz is one).  A
        # file that is large enough (ISIZE, or the compressed size where ISIZE has wrapped at 4 GiB) is decoded from block starts that
        # are searched in it; otherwise the host reader decides, and zlib refuses a file that is really damaged
        out = None
        if max(isize, n) >= ops.INFLATE_SPEC_MIN_OUT:
            try:
                out, got, found = ops.inflate_stream(comp, stages=stages)
                route = 'speculative'
                if stages is not None:
                    stages['units'] = found['units']
            except (ops.InflateForeign, IOError):
                out = None
    if out is not None:
        if got != crc or (int(out.numel()) & 0xffffffff) != isize:
            raise IOError("%s: CRC-32 / size of the decoded bytes (%08x, %d) differ from the gzip trailer (%08x, %d)"
                          % (fname, got, int(out.numel()), crc, isize))
        raw = out[:352].cpu().numpy().tobytes()
        dt, shape, off, slope, inter, spacing, origin, direction = _parse_nifti(raw, fname)
        count = shape[0] * shape[1] * shape[2]
        if dt.isnative and not _is_scaled(slope, inter) and off % dt.itemsize == 0 and hasattr(torch, dt.name):
            if off + count * dt.itemsize > int(out.numel()):
                raise IOError("%s: the file ends inside its voxels" % fname)
            if stages is not None:
                stages['path'], stages['route'] = 'device', route
            vox = out[off:off + count * dt.itemsize].view(getattr(torch, dt.name)).reshape(shape)
            return vox, tuple(float(i) for i in spacing), tuple(float(i) for i in origin), tuple(float(i) for i in direction)
    if stages is not None:
        stages['path'] = 'host'
    im = read_image(fname)
    arr = np.ascontiguousarray(im.array)
    return torch.from_numpy(arr).to(device), im.spacing, im.origin, im.direction


def _nifti_header(shape, dtype, spacing, origin, direction):
    """-> the 348 header bytes + the 4 bytes of an empty extension: a single-file NIfTI-1 ('n+1') whose voxels follow at offset 352.
    shape: [z, y, x] of the array, dtype: its numpy dtype; geometry in ITK's conventions (see the module text)."""
    dtype = np.dtype(dtype)
    nz, ny, nx = shape
    sp = np.array(spacing, dtype=np.float64)
    Rras = _LPS @ np.array(direction, dtype=np.float64).reshape(3, 3)
    t = _LPS @ np.array(origin, dtype=np.float64)
    b, c, d, qfac = _matrix_to_quaternion(Rras)
    hdr = bytearray(348)
    struct.pack_into('<i', hdr, 0, 348)
    struct.pack_into('<8h', hdr, 40, 3, nx, ny, nz, 1, 1, 1, 1)
    struct.pack_into('<hh', hdr, 70, _CODES[dtype.name], dtype.itemsize * 8)
    struct.pack_into('<8f', hdr, 76, qfac, sp[0], sp[1], sp[2], 0, 0, 0, 0)
    struct.pack_into('<3f', hdr, 108, 352.0, 1.0, 0.0)
    hdr[123] = 2                                          # millimetres
    struct.pack_into('<2h', hdr, 252, 1, 1)
    struct.pack_into('<6f', hdr, 256, b, c, d, t[0], t[1], t[2])
    M = Rras * sp
    for r in range(3):
        struct.pack_into('<4f', hdr, 280 + 16 * r, M[r, 0], M[r, 1], M[r, 2], t[r])
    hdr[344:348] = b'n+1\0'
    return bytes(hdr) + b'\0\0\0\0'


def _write_nifti(img, fname):
    arr = np.ascontiguousarray(img.array)
    if arr.dtype == np.bool_:
        arr = arr.astype(np.uint8)
    if arr.dtype.name not in _CODES:
        raise IOError("cannot write dtype %s as NIfTI" % arr.dtype)
    arr = arr.astype(arr.dtype.newbyteorder('<'))
    blob = _nifti_header(arr.shape, arr.dtype, img.spacing, img.origin, img.direction) + arr.tobytes()
    if fname.endswith('.gz'):
        with gzip.open(fname, 'wb', compresslevel=1) as f:
            f.write(blob)
    else:
        with open(fname, 'wb') as f:
            f.write(blob)


def _is_device_label_map(array, fname):
    """a uint8 tensor on a HIP device, to be written as .nii.gz: the case the device encoder serves."""
    if not fname.endswith('.nii.gz') or isinstance(array, np.ndarray):
        return False
    import torch
    return torch.is_tensor(array) and array.is_cuda and array.dtype == torch.uint8 and array.dim() == 3


def encode_label_map_device(array, spacing, origin, direction, stages=None):
    """array: uint8 device tensor [z, y, x] -> the bytes of its .nii.gz file: `_nifti_header`'s 352 bytes travel as the encoder's
    host prefix, the voxels are compressed where they are (ops.deflate_gzip) and only the compressed bytes reach the host."""
    from .. import ops
    header = _nifti_header(tuple(int(i) for i in array.shape), np.uint8, spacing, origin, direction)
    return ops.deflate_gzip(array.contiguous(), header, stages=stages)


def write_label_map_device(array, fname, spacing, origin, direction, stages=None):
    """`encode_label_map_device` into the file `fname`; the host only appends bytes to a file."""
    import time
    member = encode_label_map_device(array, spacing, origin, direction, stages)
    t0 = time.perf_counter()
    with open(fname, 'wb') as f:
        f.write(member)
    if stages is not None:
        stages['file'] = stages.get('file', 0.0) + (time.perf_counter() - t0)


def read_image(fname):
    """-> Image (array [z, y, x], spacing (x, y, z), origin, direction)."""
    if _have_sitk():
        import SimpleITK as sitk
        im = sitk.ReadImage(fname)
        return Image(sitk.GetArrayFromImage(im), im.GetSpacing(), im.GetOrigin(), im.GetDirection())
    return _read_nifti(fname)


def write_image(array, fname, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
    """Host arrays: SimpleITK when it is installed, else `_write_nifti`.  A uint8 DEVICE tensor [z, y, x] written as .nii.gz is
    compressed on the device (`write_label_map_device`), with `_write_nifti`'s header, whether or not SimpleITK is installed; any
    other device tensor is refused (there is no silent copy to the host)."""
    if _is_device_label_map(array, fname):
        return write_label_map_device(array, fname, spacing, origin, direction)
    if not isinstance(array, np.ndarray) and getattr(array, 'is_cuda', False):
        raise TypeError("write_image: only a 3-D uint8 device tensor written as .nii.gz is encoded on the device; pass a host array "
                        "for %s %s -> %s" % (getattr(array, 'dtype', '?'), tuple(getattr(array, 'shape', ())), fname))
    if _have_sitk():
        import SimpleITK as sitk
        im = sitk.GetImageFromArray(array)
        im.SetSpacing(tuple(float(i) for i in spacing))
        im.SetOrigin(tuple(float(i) for i in origin))
        im.SetDirection(tuple(float(i) for i in direction))
        sitk.WriteImage(im, fname)
        return
    _write_nifti(Image(array, spacing, origin, direction), fname)
