"""`.npz` files written from device tensors (where the reference calls `np.savez_compressed` on host copies: stored softmax
probabilities, segmentation_export.py:95-97 and ensemble_predictions.py, and the preprocessed / cropped training cases,
preprocessing.py:305 and cropping.py:174).

An .npz file is a zip archive with one member `<key>.npy` per array; a member's uncompressed stream is the .npy v1.0 header (numpy's
own `np.lib.format` builds it here, from dtype and shape) followed by the array's bytes in C order.  The header is the encoder's
host prefix, the bytes stay on the device and are DEFLATE-encoded there with run-length matches at the element size
(ops.deflate_segments: segments of at most 1 GiB, concatenated into one raw stream), and only compressed bytes reach the host.
The zip structures — local header, central directory, end record, with Zip64 fields where a size or offset does not fit 32 bits — are
written here by hand: CRC-32 and sizes stand in the local header (patched once the member is written, no data descriptor), the
file is written under a temporary name and renamed.  `np.load` reads the result; `load_npz_device` below reads a member back onto the
device, where it is inflated in parallel from the restart points the encoder leaves behind its chunks."""
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


# ---- reading: the member's compressed bytes go to the device and are inflated there (ops.inflate_raw) ----
_MAX_COMPRESSED = 2 ** 31 - 65           # what one mt_inflate_scan takes


def locate_member(fname, key):
    """-> dict(method, flags, offset, csize, usize, crc) of the member `<key>.npy`: sizes and CRC-32 from the central directory
    (`zipfile` reads it, Zip64 included), the data offset from the local header in front of the member."""
    import zipfile
    with zipfile.ZipFile(fname) as z:
        try:
            info = z.getinfo(str(key) + '.npy')
        except KeyError:
            raise KeyError("%s is not a file in the archive %s" % (key, fname))
    with open(fname, 'rb') as f:
        f.seek(info.header_offset)
        local = f.read(30)
    if len(local) != 30 or local[:4] != b'PK\x03\x04':
        raise IOError("%s: no local file header in front of member %s" % (fname, key))
    nlen, elen = struct.unpack('<HH', local[26:30])
    return {'method': info.compress_type, 'flags': info.flag_bits, 'offset': info.header_offset + 30 + nlen + elen,
            'csize': info.compress_size, 'usize': info.file_size, 'crc': info.CRC}


def parse_npy_header(first):
    """first: the leading bytes of a .npy stream -> (shape, fortran_order, dtype, header bytes), or None when they do not hold the
    whole header (its length then stands in bytes 8..11)"""
    f = io.BytesIO(bytes(first))
    try:
        version = np.lib.format.read_magic(f)
        if version == (1, 0):
            shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
        elif version == (2, 0):
            shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
        else:
            raise IOError("a .npy stream of version %s" % (version,))
    except ValueError as e:
        if len(first) < 12 or len(first) < npy_header_bytes(first):
            return None
        raise IOError("not a .npy stream: %s" % e)
    return tuple(int(s) for s in shape), bool(fortran), dtype, f.tell()


def npy_header_bytes(first):
    """the size of the .npy header whose first 12 bytes are given"""
    major = first[6]
    return 10 + struct.unpack('<H', first[8:10])[0] if major == 1 else 12 + struct.unpack('<I', first[8:12])[0]


def _load_host(fname, key, device, stages):
    import torch
    if stages is not None:
        stages['path'] = 'host'
    with np.load(fname) as z:
        arr = z[key]
    return torch.from_numpy(np.ascontiguousarray(arr)).to(device)


def load_npz_device(fname, key, device, fallback=True, stages=None):
    """`np.load(fname)[key]` as a tensor on `device`, for a file this package's writers made: only the member's compressed bytes are
    read and uploaded, they are inflated on the device, size and CRC-32 are checked against the zip header (a mismatch is an
    IOError), the .npy header comes back and is parsed by numpy's own `np.lib.format`, and the result is a view behind the header.
    A stored member, Fortran order, an object dtype or one outside the writer's list, a stream without restart points (a file
    of another writer: ops.InflateForeign) and a stream the unit rules refuse (BAD / CORRUPT / another size: a sync-flushed stream of
    another writer is one; a damaged file is then refused by zlib) are read by `np.load` and uploaded when `fallback` is set, and
    raise otherwise — unless the member holds at least ops.INFLATE_SPEC_MIN_OUT bytes and ops.inflate_stream decodes it from block
    starts it finds in the stream: a member of numpy's or any other writer's is then read on the device too.  A CRC-32
    mismatch after a successful decode is always an IOError.
    stages['path'] says 'device' or 'host' and stages['route'] 'restart' or 'speculative'; the seconds of 'file', 'upload', 'scan',
    'write' (or 'search', 'size', 'chain', 'symbols', 'windows', 'resolve'), 'crc' and 'header' are added."""
    import time
    import torch
    from .. import ops
    fname = str(fname)
    t0 = time.perf_counter()
    m = locate_member(fname, key)

    def host(why):
        if not fallback:
            raise ValueError("load_npz_device: %s[%s] is not read on the device: %s" % (fname, key, why))
        return _load_host(fname, key, device, stages)

    if m['method'] != 8 or m['flags'] & 0x9 or not 0 < m['csize'] <= _MAX_COMPRESSED:
        return host("method %d, flags %#x, %d compressed bytes" % (m['method'], m['flags'], m['csize']))
    with open(fname, 'rb') as f:
        f.seek(m['offset'])
        buf = np.fromfile(f, dtype=np.uint8, count=m['csize'])
    if buf.size != m['csize']:
        raise IOError("%s: member %s is cut short" % (fname, key))
    t1 = time.perf_counter()
    comp = torch.from_numpy(buf).to(device)
    if stages is not None:
        torch.cuda.synchronize(comp.device)
        stages['file'] = stages.get('file', 0.0) + (t1 - t0)
        stages['upload'] = stages.get('upload', 0.0) + (time.perf_counter() - t1)
    route = 'restart'
    try:
        out, crc, _ = ops.inflate_raw(comp, n_out=m['usize'], stages=stages)
    except (ops.InflateForeign, IOError) as e:
        # InflateForeign: no restart points.  BAD / CORRUPT / a size mismatch are verdicts of the UNIT rules: a valid stream of another
        # writer that holds empty stored blocks without a dictionary reset behind them (zlib's Z_SYNC_FLUSH, pigz) fails them too.
        # A member that is large enough is decoded from block starts that are searched in it; what that refuses as
        # well goes to zlib, which decides what is damaged
        out = None
        if m['usize'] >= ops.INFLATE_SPEC_MIN_OUT:
            try:
                out, crc, found = ops.inflate_stream(comp, n_out=m['usize'], stages=stages)
                route = 'speculative'
                if stages is not None:
                    stages['units'] = found['units']
            except (ops.InflateForeign, IOError):
                out = None
        if out is None:
            if isinstance(e, IOError) and not fallback:
                raise
            return host(str(e))
    t2 = time.perf_counter()
    if crc != m['crc']:
        raise IOError("%s: CRC-32 of member %s is %08x, its header says %08x" % (fname, key, crc, m['crc']))
    first = out[:min(m['usize'], 4096)].cpu().numpy().tobytes()
    head = parse_npy_header(first)
    if head is None and len(first) >= 12:
        head = parse_npy_header(out[:min(m['usize'], npy_header_bytes(first))].cpu().numpy().tobytes())
    if head is None:
        raise IOError("%s: member %s is no .npy stream" % (fname, key))
    shape, fortran, dtype, hbytes = head
    count = int(np.prod(shape, dtype=np.int64))
    if fortran or dtype.hasobject or not dtype.isnative or dtype.name not in _DTYPES or hbytes % dtype.itemsize \
            or not hasattr(torch, dtype.name):
        return host("%s, fortran_order %s" % (dtype, fortran))
    if hbytes + count * dtype.itemsize != m['usize']:
        raise IOError("%s: member %s holds %d bytes, its header describes %d" % (fname, key, m['usize'], hbytes + count * dtype.itemsize))
    t = out[hbytes:].view(getattr(torch, dtype.name)).reshape(shape)
    if stages is not None:
        stages['path'], stages['route'] = 'device', route
        stages['header'] = stages.get('header', 0.0) + (time.perf_counter() - t2)
    return t


def peek_npy_header(fname, key):
    """(shape, fortran_order, dtype) of member `<key>.npy` without inflating it: the first compressed bytes of the member are
    read and only the .npy header at the head of the stream is decoded (zlib, a few hundred bytes); None where that cannot be done."""
    import zlib
    try:
        m = locate_member(fname, key)
        if m['method'] not in (0, 8) or m['flags'] & 0x1:
            return None
        with open(fname, 'rb') as f:
            f.seek(m['offset'])
            buf = f.read(min(m['csize'], 1 << 16))
        first = buf[:4096] if m['method'] == 0 else zlib.decompressobj(-15).decompress(buf, 4096)
        head = parse_npy_header(first)
    except (IOError, KeyError, zlib.error):
        return None
    return None if head is None else head[:3]
