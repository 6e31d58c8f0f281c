"""Shared by test_bgzf_format.py and test_bgzf_gpu.py: a pure-Python BGZF
writer and walk (the tests' own statement of the format, independent of the
library), the files both tests index, and device-buffer helpers."""
import ctypes
import struct
import zlib

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
EDATA, ECAP = -5, -4


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def stored(data, final=1):
    return bytes([final]) + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data


def member(data=b"", level=6, payload=None, extra=b"", isize=None, crc=None, bsize=None):
    """one gzip member: `extra` holds subfields written before BC"""
    if payload is None:
        payload = raw_deflate(data, level)
    xlen = len(extra) + 6
    size = 12 + xlen + len(payload) + 8
    bs = size - 1 if bsize is None else bsize
    return (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", xlen) + extra +
            b"BC" + struct.pack("<HH", 2, bs) + payload +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc,
                        len(data) if isize is None else isize))


def walk(buf):
    """-> (rows of (offset, payload offset, payload size, isize, crc), eof,
    status): the chain from offset 0; status 0 or EDATA"""
    rows, off, n = [], 0, len(buf)
    while off < n:
        h = buf[off:off + 12]
        if len(h) < 12 or h[:4] != b"\x1f\x8b\x08\x04":
            return rows, False, EDATA
        xlen = h[10] | h[11] << 8
        ex = buf[off + 12:off + 12 + xlen]
        if xlen < 6 or len(ex) < xlen:
            return rows, False, EDATA
        q, bs = 0, None
        while q + 4 <= xlen:
            slen = ex[q + 2] | ex[q + 3] << 8
            if ex[q:q + 2] == b"BC" and slen == 2:
                if q + 6 <= xlen:
                    bs = ex[q + 4] | ex[q + 5] << 8
                break
            q += 4 + slen
        if bs is None or bs + 1 < xlen + 20 or off + bs + 1 > n:
            return rows, False, EDATA
        crc, isz = struct.unpack("<II", buf[off + bs + 1 - 8:off + bs + 1])
        rows.append((off, off + 12 + xlen, bs + 1 - xlen - 20, isz, crc))
        off += bs + 1
    return rows, bool(rows) and buf[rows[-1][0]:] == EOF, 0


def pattern(n, seed):
    """n compressible bytes"""
    out = bytearray()
    x = seed * 2654435761 & 0xffffffff
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7fffffff
        out += b"the quick brown fox %d jumps " % (x % 97)
    return bytes(out[:n])


def variable_members():
    datas = [b"A", pattern(4097, 1), pattern(65280, 2), bytes(65536)]
    return datas, [member(d) for d in datas]


def two_fakes():
    """two fake member headers inside stored payloads: the first one's
    successor is the true second member (two predecessors for one node), the
    other's is no candidate"""
    def fake(bs):
        return b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bs)
    n0 = 100
    off1 = 18 + 5 + n0 + 8                      # where member 1 starts
    posa = 18 + 5 + 10                          # fake A's position
    d0 = bytes(10) + fake(off1 - posa - 1) + bytes(n0 - 28)
    d1 = bytes(7) + fake(30) + bytes(200)       # fake B: its end lands in these zeros
    ms = [member(d0, payload=stored(d0)), member(d1, payload=stored(d1)), member(pattern(500, 3))]
    return b"".join(ms) + EOF


def cases():
    """name -> file; the expected index is walk(file)"""
    datas, ms = variable_members()
    good = b"".join(ms)
    c = {}
    c["variable_eof"] = good + EOF
    c["variable_noeof"] = good
    c["empty_mid"] = ms[1] + member(b"") + ms[0] + EOF
    c["extra_before_bc"] = (member(pattern(300, 4), extra=b"XY\x03\x00abc") +
                            member(pattern(10, 5), extra=b"Q1\x00\x00RG\x02\x00zz") + EOF)
    two = ms[0] + ms[1] + ms[0]
    o2 = len(ms[0]) + len(ms[1])
    c["cut_header"] = two[:o2 + 5]
    c["cut_payload"] = (ms[0] + ms[1])[:len(ms[0]) + 40]
    c["cut_trailer"] = (ms[0] + ms[1])[:-3]
    c["bsize_past_end"] = ms[0] + member(pattern(50, 6), bsize=4000) + EOF
    inner = member(pattern(40, 7))
    d = b"zz" + inner + b"yy"
    c["fake_in_stored"] = ms[0] + member(d, payload=stored(d)) + EOF
    c["two_fakes"] = two_fakes()
    c["minimal_300"] = b"".join(member(b"" if i % 3 else b"x") for i in range(300))
    c["only_eof"] = EOF
    c["empty"] = b""
    c["garbage"] = bytes(range(64))
    return c


class Dev:
    """hipMalloc'ed buffers; data placed so that it ends at (or, when 16-byte
    alignment is asked for, within 15 bytes of) the allocation's last page"""
    PAGE = 4096

    def __init__(self):
        self.L = ctypes.CDLL("libamdhip64.so")
        self.L.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.L.hipFree.argtypes = [ctypes.c_void_p]
        self.L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.L.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        self.bufs = []

    def tail(self, n, align=1):
        size = max(self.PAGE, -(-(n + align) // self.PAGE) * self.PAGE)
        p = ctypes.c_void_p()
        assert self.L.hipMalloc(ctypes.byref(p), size) == 0
        self.bufs.append(p.value)
        assert self.L.hipMemset(p, 0xA5, size) == 0
        return (p.value + size - n) & ~(align - 1)

    def put(self, data, align=16):
        d = self.tail(len(data), align)
        if data:
            b = ctypes.create_string_buffer(bytes(data), len(data))
            assert self.L.hipMemcpy(d, b, len(data), 1) == 0
        return d

    def get(self, d, n):
        assert self.L.hipDeviceSynchronize() == 0
        b = ctypes.create_string_buffer(max(n, 1))
        if n:
            assert self.L.hipMemcpy(b, d, n, 2) == 0
        return b.raw[:n]

    def get_array(self, d, n, fmt):
        return list(struct.unpack("<%d%s" % (n, fmt), self.get(d, n * struct.calcsize(fmt))))

    def free(self):
        self.L.hipDeviceSynchronize()
        for p in self.bufs:
            self.L.hipFree(p)
        self.bufs = []


def device_index(J, H, buf, maxblocks):
    """jdgpu_bgzf_index_device -> (rows, eof, status)"""
    d = H.put(buf)
    m = max(maxblocks, 1)
    mo, po = H.tail(8 * m, 8), H.tail(8 * m, 8)
    ps, isz, crc = H.tail(4 * m, 4), H.tail(4 * m, 4), H.tail(4 * m, 4)
    nb, eof = H.tail(4, 4), H.tail(4, 4)
    r = J.bgzf_index_device(d, len(buf), maxblocks, mo, po, ps, isz, crc, nb, eof)
    k = H.get_array(nb, 1, "I")[0]
    assert k <= maxblocks
    rows = list(zip(H.get_array(mo, k, "Q"), H.get_array(po, k, "Q"), H.get_array(ps, k, "I"),
                    H.get_array(isz, k, "I"), H.get_array(crc, k, "I")))
    return rows, bool(H.get_array(eof, 1, "I")[0]), r


def device_round_trip(J, H, data, level, blocksize=65280, out_align=16):
    """bgzf_deflate_device + bgzf_inflate_device with every caller buffer of
    exactly its size at a page end -> (file, member offsets, bytes, errors, rc)"""
    n = len(data)
    nb = -(-n // blocksize)
    cap = J.bgzf_bound(n, blocksize)
    d_in = H.put(data)
    d_out = H.tail(cap)
    d_bo = H.tail(8 * max(nb, 1), 8)
    d_tot = H.tail(8, 8)
    J.bgzf_deflate_device(d_in, n, d_out, cap, d_bo, d_tot, level=level, blocksize=blocksize)
    total = H.get_array(d_tot, 1, "Q")[0]
    assert total <= cap
    comp = H.get(d_out, total)
    offs = H.get_array(d_bo, nb, "Q")
    d_c = H.put(comp)
    d_back = H.tail(n, out_align)
    d_err = H.tail(4 * (nb + 1), 4)
    d_t2 = H.tail(8, 8)
    rc = J.bgzf_inflate_device(d_c, total, d_back, n, d_t2, d_err, nb + 1)
    assert H.get_array(d_t2, 1, "Q")[0] == n
    return comp, offs, H.get(d_back, n), H.get_array(d_err, nb + 1, "i"), rc
