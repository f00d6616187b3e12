"""Row f.4: gnark-crypto's point bytes, decoded and encoded on the device (nlx_bn254_g1_decode / g2_decode / g1_encode / g2_encode;
csrc/bn254_codec.hpp / .hip), and the big-endian scalars and slices the containers around them are made of
(kzg.SRS in bn254_plonk.py, groth16.ProvingKey in bn254_groth16.py).  The place of record for every byte rule is
tools/gnark_bytes_model.py; the rules are recalled from gnark v0.9 / gnark-crypto and unpinned, like the rest of row f.4.

Bytes are `bytes` / bytearray / memoryview, numpy uint8 arrays or uint8 device tensors; words are (n, 8) / (n, 16) uint64 numpy
arrays or 8-byte integer device tensors (G1Affine / G2Affine as they lie in memory, Montgomery; all zero = the point at infinity).
A device tensor in gives a device tensor out, as does device="cuda:k".

The library works on its context's own stream, which does not wait for torch's: before a call, torch's current stream on the
tensors' device is synchronised (a fill or a copy still queued there - torch.zeros, a device-to-device hipMemcpy - would
otherwise land under or after the kernels), and device outputs made here come from torch.empty: the kernels write every byte and
word, a bad point's included.  Every call returns with the context's stream drained."""
import numpy as np

from ._lib import NlxError, dll

POINTS_COMPRESSED, POINTS_RAW, POINTS_NO_SUBGROUP = 1, 2, 4
POINT_OK, POINT_BAD_FLAG, POINT_RANGE, POINT_BAD_INFINITY, POINT_OFF_CURVE, POINT_NOT_IN_SUBGROUP = range(6)
POINT_REASONS = {POINT_BAD_FLAG: "the flag bits are not valid in this mode", POINT_RANGE: "a coordinate is not below q",
                 POINT_BAD_INFINITY: "the infinity flag with another bit set",
                 POINT_OFF_CURVE: "not on the curve (no square root, or a raw point off the curve)",
                 POINT_NOT_IN_SUBGROUP: "not in the subgroup of order r"}
G1_BYTES, G2_BYTES = 32, 64           # compressed; raw: twice that
NLX_E_INVAL = -1


def point_bytes(g2, raw):
    return (G2_BYTES if g2 else G1_BYTES) * (2 if raw else 1)


def _settle(*buffers):
    """torch's queued work on the device tensors among `buffers` is done before the library touches them"""
    for b in buffers:
        if hasattr(b, "data_ptr") and b.is_cuda:
            import torch
            torch.cuda.current_stream(b.device).synchronize()
            return


def _bytes_in(data):
    """(object kept alive, address, length) of the caller's bytes"""
    if hasattr(data, "data_ptr"):
        if not data.is_contiguous() or data.element_size() != 1:
            raise TypeError("expected a contiguous uint8 tensor")
        return data, data.data_ptr(), data.numel()
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    return a, a.ctypes.data, a.size


def _words_in(points, width):
    if hasattr(points, "data_ptr"):
        if not points.is_contiguous() or points.element_size() != 8 or points.is_floating_point() or points.numel() % width:
            raise TypeError("expected a contiguous (n, %d) tensor of 8-byte integers" % width)
        return points, points.data_ptr(), points.numel() // width
    a = np.ascontiguousarray(points, dtype=np.uint64)
    if a.size % width:
        raise ValueError("expected (n, %d) words" % width)
    return a, a.ctypes.data, a.size // width


def _decode(ctx, g2, data, raw, subgroup, out, status, device):
    held, src, length = _bytes_in(data)         # held: a converted copy, where one was made, lives until the call is over
    size, width = point_bytes(g2, raw), 16 if g2 else 8
    if length % size:
        raise ValueError("%d bytes are no whole number of %d-byte points" % (length, size))
    n = length // size
    on_device = device is not None or hasattr(data, "data_ptr")
    if out is None:
        if on_device:
            import torch
            out = torch.empty((n, width), dtype=torch.int64, device=device if device is not None else data.device)
        else:
            out = np.zeros((n, width), dtype=np.uint64)
    _, dst, rows = _words_in(out, width)
    if rows != n:
        raise ValueError("out holds %d points, the bytes %d" % (rows, n))
    st_ptr = None
    if status is not None:
        if hasattr(status, "data_ptr"):
            if status.numel() != n or status.element_size() != 4 or not status.is_contiguous():
                raise TypeError("status: n contiguous 4-byte integers")
            st_ptr = status.data_ptr()
        else:
            if status.dtype != np.uint32 or status.size != n or not status.flags["C_CONTIGUOUS"]:
                raise TypeError("status: a C-contiguous uint32 array of n words")
            st_ptr = status.ctypes.data
    flags = (POINTS_RAW if raw else POINTS_COMPRESSED) | (0 if subgroup or not g2 else POINTS_NO_SUBGROUP)
    _settle(data, out, status)
    fn = dll.nlx_bn254_g2_decode if g2 else dll.nlx_bn254_g1_decode
    ctx.check(fn(ctx.handle, src if n else None, n, flags, dst if n else None, st_ptr if n else None))
    del held
    return out


def bn254_g1_decode(ctx, data, raw=False, out=None, status=None, device=None):
    """G1Affine.SetBytes over n points (nlx_bn254_g1_decode): 32 n bytes (raw: 64 n) -> (n, 8) words.  A bad point raises NlxError
    (NLX_E_INVAL) naming the lowest bad index and its reason; `out` and `status` (n uint32 words: POINT_*), when handed in, are
    filled all the same - a bad point's words are zero."""
    return _decode(ctx, False, data, raw, True, out, status, device)


def bn254_g2_decode(ctx, data, raw=False, subgroup=True, out=None, status=None, device=None):
    """G2Affine.SetBytes over n points (nlx_bn254_g2_decode): 64 n bytes (raw: 128 n) -> (n, 16) words; subgroup=False leaves the
    test of the order-r subgroup out."""
    return _decode(ctx, True, data, raw, subgroup, out, status, device)


def _encode(ctx, g2, points, raw, out, device):
    held, src, n = _words_in(points, 16 if g2 else 8)      # held: as in _decode
    size = point_bytes(g2, raw)
    on_device = device is not None or hasattr(points, "data_ptr")
    made = out is None
    if made:
        if on_device:
            import torch
            out = torch.empty(n * size, dtype=torch.uint8, device=device if device is not None else points.device)
        else:
            out = np.zeros(n * size, dtype=np.uint8)
    _, dst, length = _bytes_in(out)
    if length != n * size:
        raise ValueError("out holds %d bytes, the points need %d" % (length, n * size))
    fn = dll.nlx_bn254_g2_encode if g2 else dll.nlx_bn254_g1_encode
    _settle(points, out)
    ctx.check(fn(ctx.handle, src if n else None, n, POINTS_RAW if raw else POINTS_COMPRESSED, dst if n else None))
    del held
    return out.tobytes() if made and not on_device else out


def bn254_g1_encode(ctx, points, raw=False, out=None, device=None):
    """G1Affine.Bytes() (raw: RawBytes()) over n points (nlx_bn254_g1_encode): `bytes` for host words, a uint8 device tensor for
    device words or device="cuda:k", or `out` (a numpy uint8 array / uint8 tensor of the right length) filled.  The curve is not
    tested; a coordinate that is not below q raises NlxError (NLX_E_RANGE) naming the index."""
    return _encode(ctx, False, points, raw, out, device)


def bn254_g2_encode(ctx, points, raw=False, out=None, device=None):
    """G2Affine.Bytes() (raw: RawBytes()) over n points (nlx_bn254_g2_encode)"""
    return _encode(ctx, True, points, raw, out, device)


# ---- the scalars and slices of gnark's containers (tools/gnark_bytes_model.py rule 8) ----
def u32(x):
    return int(x).to_bytes(4, "big")


def u64(x):
    return int(x).to_bytes(8, "big")


def slice_bytes(ctx, g2, points, raw):
    """a slice of points: a big-endian uint32 count and the points, encoded in one call"""
    _, _, n = _words_in(points, 16 if g2 else 8)
    body = _encode(ctx, g2, points, raw, None, None)
    return u32(n) + (body if isinstance(body, bytes) else body.cpu().numpy().tobytes())


class Reader:
    """Walks a container's bytes.  Every read names its section: short data raises NlxError (NLX_E_INVAL) "truncated in <section>",
    a bad point "<section> point <i>: ..." with the codec's own reason."""

    def __init__(self, ctx, data, raw, device=None):
        self.ctx, self.raw, self.device, self.at = ctx, raw, device, 0
        self.data = memoryview(data if isinstance(data, (bytes, bytearray, memoryview)) else bytes(data))

    def take(self, n, section):
        if self.at + n > len(self.data):
            raise NlxError(NLX_E_INVAL, "truncated in %s: %d bytes wanted at offset %d, %d left" % (section, n, self.at, len(self.data) - self.at))
        out = self.data[self.at:self.at + n]
        self.at += n
        return out

    def u32(self, section):
        return int.from_bytes(self.take(4, section), "big")

    def u64(self, section):
        return int.from_bytes(self.take(8, section), "big")

    def _decode(self, g2, data, section, single, device):
        """the codec's status words say which point is bad and why: nothing is read out of the library's message"""
        status = np.zeros(len(data) // point_bytes(g2, self.raw), dtype=np.uint32)
        try:
            return _decode(self.ctx, g2, data, self.raw, True, None, status, device)
        except NlxError as e:
            bad = np.nonzero(status)[0]
            if e.code != NLX_E_INVAL or not len(bad):
                raise
            index = int(bad[0])
            where = section if single else "%s point %d" % (section, index)
            raise NlxError(NLX_E_INVAL, "%s: %s" % (where, POINT_REASONS.get(int(status[index]), "status %d" % status[index]))) from None

    def point(self, g2, section):
        """one point -> its words (numpy)"""
        return self._decode(g2, self.take(point_bytes(g2, self.raw), section), section, True, None)[0]

    def points(self, g2, section, device=False):
        """a slice -> (n, width) words, in one call of the codec; device=True: on the reader's device, when it has one"""
        n = self.u32(section + " count")
        size = point_bytes(g2, self.raw)
        if self.at + n * size > len(self.data):
            raise NlxError(NLX_E_INVAL, "truncated in %s: %d points of %d bytes wanted, %d bytes left" % (section, n, size, len(self.data) - self.at))
        return self._decode(g2, self.take(n * size, section), section, False, self.device if device else None)

    def bools(self, section):
        n = self.u32(section + " count")
        a = np.frombuffer(self.take(n, section), dtype=np.uint8)
        if n and a.max() > 1:
            raise NlxError(NLX_E_INVAL, "%s: a byte that is neither 0 nor 1" % section)
        return a.copy()

    def end(self, what):
        if self.at != len(self.data):
            raise NlxError(NLX_E_INVAL, "%s: %d trailing bytes" % (what, len(self.data) - self.at))


def container_is_raw(data, before, what):
    """the mode of a container, from the flag bits of its first point `what` (never the point at infinity).  before: the
    (section, size) pairs that precede it - a file that ends inside one of them is refused naming that one"""
    at = 0
    for section, size in before:
        if len(data) < at + size:
            raise NlxError(NLX_E_INVAL, "truncated in %s: %d bytes wanted at offset %d, %d left" % (section, size, at, len(data) - at))
        at += size
    if len(data) <= at:
        raise NlxError(NLX_E_INVAL, "truncated in %s: a point wanted at offset %d, 0 bytes left" % (what, at))
    flag = data[at] >> 6
    if flag == 1:
        raise NlxError(NLX_E_INVAL, "%s is the point at infinity" % what)
    return flag == 0
