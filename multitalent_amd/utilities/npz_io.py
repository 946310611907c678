"""`.npz` files written from device tensors (where the reference calls `np.savez_compressed` on host copies: stored softmax
probabilities, segmentation_export.py:95-97 and ensemble_predictions.py, and the preprocessed / cropped training cases,
preprocessing.py:305 and cropping.py:174).

An .npz file is a zip archive with one member `<key>.npy` per array; a member's uncompressed stream is the .npy v1.0 header (numpy's
own `np.lib.format` builds it here, from dtype and shape) followed by the array's bytes in C order.  The header is the encoder's
host prefix, the bytes stay on the device and are DEFLATE-encoded there with run-length matches at the element size
(ops.deflate_segments: segments of at most 1 GiB, concatenated into one raw stream), and only compressed bytes reach the host.
The zip structures — local header, central directory, end record, with Zip64 fields where a size or offset does not fit 32 bits — are
written here by hand: CRC-32 and sizes stand in the local header (patched once the member is written, no data descriptor), the
file is written under a temporary name and renamed.  `np.load` reads the result; reading and inflating are not part of this."""
import io
import os
import struct

import numpy as np

_LIMIT = 0xffffffff
_Z64_MARGIN = 1 << 20          # compressed bytes exceed the input by at most 10 per 64 KiB chunk (all chunks stored): far below this
_DATE, _TIME = (1 << 5) | 1, 0  # 1980-01-01 00:00: the same tensors give the same file
_DTYPES = ('float16', 'float32', 'float64', 'uint8', 'int8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64')


class HostBodies(object):
    """compressed bytes of one member that are already on the host: an iterable of bodies plus the CRC-32 of the uncompressed
    stream (what ops.deflate_segments is for a device tensor)"""

    def __init__(self, bodies, crc):
        self.bodies, self.crc = list(bodies), crc & 0xffffffff
        self.compressed = sum(len(b) for b in self.bodies)

    def __iter__(self):
        return iter(self.bodies)


def npy_header(dtype, shape):
    """the .npy v1.0 header (magic, version, padded dict) of a C-ordered array, as numpy writes it"""
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, {'descr': np.lib.format.dtype_to_descr(np.dtype(dtype)), 'fortran_order': False,
                                             'shape': tuple(int(s) for s in shape)})
    return f.getvalue()


def _numpy_dtype(t):
    name = str(t.dtype).replace('torch.', '')
    if name not in _DTYPES:
        raise TypeError("save_npz_device: %s tensors are not written (float16/32/64 and the integer types of 1, 2, 4 or 8 bytes are)" % t.dtype)
    return np.dtype(name)


def _local_header(name, crc, csize, usize, zip64):
    extra = struct.pack('<HHQQ', 1, 16, usize, csize) if zip64 else b''
    if zip64:
        csize = usize = _LIMIT
    return struct.pack('<4sHHHHHIIIHH', b'PK\x03\x04', 45 if zip64 else 20, 0, 8, _TIME, _DATE, crc, csize, usize, len(name),
                       len(extra)) + name + extra


def _central_header(name, crc, csize, usize, offset, force):
    fields = []
    if force or usize >= _LIMIT or csize >= _LIMIT:
        fields += [usize, csize]
        usize = csize = _LIMIT
    if force or offset >= _LIMIT:
        fields.append(offset)
        offset = _LIMIT
    extra = struct.pack('<HH%dQ' % len(fields), 1, 8 * len(fields), *fields) if fields else b''
    ver = 45 if fields else 20
    return struct.pack('<4sHHHHHHIIIHHHHHII', b'PK\x01\x02', ver, ver, 0, 8, _TIME, _DATE, crc, csize, usize, len(name), len(extra),
                       0, 0, 0, 0o600 << 16, offset) + name + extra


def _end_records(count, cd_size, cd_offset, force):
    out = b''
    if force or count >= 0xffff or cd_size >= _LIMIT or cd_offset >= _LIMIT:
        out += struct.pack('<4sQHHIIQQQQ', b'PK\x06\x06', 44, 45, 45, 0, 0, count, count, cd_size, cd_offset)
        out += struct.pack('<4sIQI', b'PK\x06\x07', 0, cd_offset + cd_size, 1)
        count, cd_size, cd_offset = min(count, 0xffff), min(cd_size, _LIMIT), min(cd_offset, _LIMIT)
        if force:
            count, cd_size, cd_offset = 0xffff, _LIMIT, _LIMIT
    return out + struct.pack('<4sHHHHIIH', b'PK\x05\x06', 0, 0, count, count, cd_size, cd_offset, 0)


def write_npz_members(fname, members, _force_zip64=False):
    """members: [(key, n, bodies)] — n = uncompressed bytes of the member `<key>.npy`, bodies = an iterable of pieces of its raw
    DEFLATE stream that has .crc once it is exhausted (ops.deflate_segments, HostBodies).  Each piece is written and dropped before
    the next is asked for."""
    fname = str(fname)
    if not fname.endswith('.npz'):
        fname += '.npz'
    tmp = fname + '.tmp%d' % os.getpid()
    central = []
    try:
        with open(tmp, 'wb') as f:
            for key, n, bodies in members:
                name = (str(key) + '.npy').encode('utf-8')
                zip64 = _force_zip64 or n >= _LIMIT - _Z64_MARGIN
                offset = f.tell()
                f.write(_local_header(name, 0, 0, 0, zip64))
                start = f.tell()
                for b in bodies:
                    f.write(b)
                end = f.tell()
                f.seek(offset)
                f.write(_local_header(name, bodies.crc, end - start, n, zip64))
                f.seek(end)
                central.append(_central_header(name, bodies.crc, end - start, n, offset, _force_zip64))
            cd_offset = f.tell()
            for c in central:
                f.write(c)
            f.write(_end_records(len(central), f.tell() - cd_offset, cd_offset, _force_zip64))
        os.replace(tmp, fname)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return fname


def _device_members(tensors, chunk, segment_bytes, stages):
    from .. import ops
    out = []
    for key, t in tensors.items():
        if not hasattr(t, 'is_cuda') or not t.is_cuda:
            raise TypeError("save_npz_device: '%s' is not a device tensor; host arrays are written with np.savez_compressed" % key)
        dt = _numpy_dtype(t)
        t = t.contiguous()
        header = npy_header(dt, t.shape)
        kw = {} if segment_bytes is None else {'segment_bytes': segment_bytes}
        seg = ops.deflate_segments(t, header, chunk or ops.DEFLATE_CHUNK, dt.itemsize, stages=stages, **kw)
        out.append((key, seg.n, seg))
    return out


def save_npz_device(fname, _force_zip64=False, _chunk=None, _segment_bytes=None, _stages=None, **device_tensors):
    """`np.savez_compressed(fname, **arrays)` for device tensors: one member per tensor, compressed on the device, never copied
    to the host uncompressed.  A non-contiguous tensor is made contiguous on the device.  -> the file name (with .npz)."""
    return write_npz_members(fname, _device_members(device_tensors, _chunk, _segment_bytes, _stages), _force_zip64)


def encode_npz_device(_stages=None, **device_tensors):
    """The device half of save_npz_device alone: -> members with their compressed bytes on the host, for `write_npz_members` on
    another thread (an executor that must not touch the device)."""
    out = []
    for key, n, seg in _device_members(device_tensors, None, None, _stages):
        bodies = list(seg)
        out.append((key, n, HostBodies(bodies, seg.crc)))
    return out
