"""BGZF on the GPU: every-block-final deflate framed into gzip members on the
device, the device index against the host walk, and the indexed inflate with
its per-member verification."""
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bgzf_cases as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 65280
MAXPAY = 65510
CASES = B.cases()


def corpus(J):
    """four 65,280-byte blocks (text, random, runs, text) and a 1,234-byte tail"""
    rng = np.random.default_rng(20240607)
    runs = np.repeat(rng.integers(0, 256, 2048, dtype=np.uint8), 32)[:BS]
    parts = [J.corpus_text(BS, seed=11), rng.integers(0, 256, BS, dtype=np.uint8), runs,
             J.corpus_text(BS, seed=12), J.corpus_text(1234, seed=13)]
    return b"".join(p.tobytes() for p in parts)


@pytest.fixture(scope="module")
def data(engine):
    return corpus(engine)


_REF = {}


def ref_payloads(oracle, data, level, bs=BS):
    """per block: the oracle's stream of a fresh deflator with DEFLT_END"""
    key = (hash(data), level, bs)
    if key not in _REF:
        _REF[key] = [oracle.deflate(data[o:o + bs], level, flush=1) for o in range(0, len(data), bs)]
    return _REF[key]


def check_file(J, oracle, data, out, offs, level, bs=BS):
    assert gzip.decompress(out) == data
    assert out.endswith(B.EOF)
    rows, eof, st = B.walk(out)
    assert st == 0 and eof
    blocks = [data[o:o + bs] for o in range(0, len(data), bs)]
    assert len(rows) == len(blocks) + 1
    assert offs == [r[0] for r in rows[:-1]]
    refs = ref_payloads(oracle, data, level, bs)
    sizes = [b[0] - a[0] for a, b in zip(rows, rows[1:])]
    assert max(sizes) <= 65536
    for blk, ref, (off, po, ps, isz, crc) in zip(blocks, refs, rows):
        want = ref if len(ref) <= MAXPAY else B.stored(blk)
        assert out[po:po + ps] == want
        assert crc == zlib.crc32(blk) and isz == len(blk)
        assert po == off + 18


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_encode(engine, oracle, data, level):
    offs = []
    out = engine.bgzf_compress(data, level=level, offsets=offs)
    check_file(engine, oracle, data, out, offs, level)


def test_level1_takes_both_paths(oracle, data):
    """from the oracle alone: at level 1 the random block's stream cannot fit
    a member and the text blocks' can, so test_encode[1] covers the fallback"""
    n = [len(p) for p in ref_payloads(oracle, data, 1)]
    assert n[1] > MAXPAY and n[0] <= MAXPAY and n[3] <= MAXPAY


@pytest.mark.parametrize("n,bs", [(0, BS), (1, BS), (BS, BS), (3 * 4096 + 5, 4096)])
def test_encode_sizes(engine, oracle, n, bs):
    d = engine.corpus_text(max(n, 16), seed=21).tobytes()[:n]
    offs = []
    out = engine.bgzf_compress(d, level=6, blocksize=bs, offsets=offs)
    if n == 0:
        assert out == B.EOF and offs == []
    else:
        check_file(engine, oracle, d, out, offs, 6, bs)


def test_encode_errors(engine, data):
    E = engine.engine
    for bs in (65296, 100):
        with pytest.raises(engine.BgzfError) as ex:
            engine.bgzf_compress(data[:1000], blocksize=bs, cap=70000)
        assert ex.value.code == E.JDGPU_EINVAL
    out = engine.bgzf_compress(data[:100000])
    with pytest.raises(engine.BgzfError) as ex:
        engine.bgzf_compress(data[:100000], cap=len(out) - 1)
    assert ex.value.code == E.JDGPU_ECAP
    assert engine.bgzf_compress(data[:100000], cap=len(out)) == out


@pytest.mark.parametrize("level", range(10))
def test_every_block_final(engine, oracle, level):
    bs = 16384
    d = engine.corpus_mixed(2 * bs + 777, seed=31, blocksize=bs).tobytes()
    out = engine.bgzf_compress(d, level=level, blocksize=bs)
    rows, eof, st = B.walk(out)
    assert st == 0 and eof and len(rows) == 4
    for i, (off, po, ps, isz, crc) in enumerate(rows[:3]):
        assert out[po:po + ps] == oracle.deflate(d[i * bs:(i + 1) * bs], level, flush=1), i
    # the existing mode at the same commit: the last block alone is final
    got = engine.deflate_blocks(d, level=level, blocksize=bs)
    assert got == oracle.deflate_blocks(d, level=level, blocksize=bs)


@pytest.fixture
def dev():
    H = B.Dev()
    yield H
    H.free()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_index_equals_walk(engine, dev, name):
    buf = CASES[name]
    want = B.walk(buf)
    assert B.device_index(engine, dev, buf, len(want[0]) + 3) == want
    # capacity exactly the number of members
    if want[0]:
        assert B.device_index(engine, dev, buf, len(want[0])) == want


def test_device_index_capacity(engine, dev):
    buf = CASES["variable_eof"]
    rows, eof, st = B.walk(buf)
    got = B.device_index(engine, dev, buf, len(rows) - 1)
    assert got == (rows[:-1], False, B.ECAP)


def test_device_index_of_own_output(engine, dev, data):
    out = engine.bgzf_compress(data, level=1)
    assert B.device_index(engine, dev, out, 8) == B.walk(out)


def counts(J, fn):
    J.prof_enable(True)
    try:
        r = fn()
        return r, J.prof_read()
    finally:
        J.prof_enable(False)


def test_round_trip_without_copy(engine, data):
    out = engine.bgzf_compress(data, level=6)
    back, prof = counts(engine, lambda: engine.bgzf_decompress(out))
    assert back == data
    assert "k_compact" not in prof and prof["k_checksum_members"][1] >= 1


def test_foreign_file_gathers(engine):
    datas, ms = B.variable_members()
    buf = CASES["empty_mid"][:-len(B.EOF)] + b"".join(ms) + B.EOF
    want = datas[1] + datas[0] + b"".join(datas)
    errs = []
    back, prof = counts(engine, lambda: engine.bgzf_decompress(buf, errors=errs))
    assert back == want and errs == [0] * 8
    assert prof["k_compact"][1] >= 1


def five_members():
    datas = [B.pattern(3000 + 977 * i, 40 + i) for i in range(5)]
    ms = [B.member(d) for d in datas]
    return datas, ms


def decode_fail(J, buf):
    with pytest.raises(J.BgzfError) as ex:
        J.bgzf_decompress(buf)
    assert ex.value.code == J.engine.JDGPU_EDATA
    return ex.value


def test_flipped_payload_bit(engine):
    datas, ms = five_members()
    bad = bytearray(ms[2])
    bad[18 + len(bad) // 3] ^= 0x10
    ex = decode_fail(engine, b"".join(ms[:2]) + bytes(bad) + b"".join(ms[3:]) + B.EOF)
    assert [bool(e) for e in ex.errors] == [False, False, True, False, False, False]
    o = 0
    for i, d in enumerate(datas):
        if i != 2:
            assert ex.data[o:o + len(d)] == d, i
        o += len(d)


def test_flipped_crc_and_wrong_isize(engine):
    E = engine.engine
    datas, ms = five_members()
    bad = bytearray(ms[1])
    bad[-8] ^= 1
    ex = decode_fail(engine, ms[0] + bytes(bad) + ms[2] + B.EOF)
    assert ex.errors == [0, E.JDGPU_EMEMBERCRC, 0, 0]
    bad = bytearray(ms[3])
    bad[-4:] = struct.pack("<I", len(datas[3]) - 1)
    ex = decode_fail(engine, ms[0] + bytes(bad) + B.EOF)
    assert ex.errors == [0, E.JDGPU_EMEMBERSIZE, 0]


def test_broken_chain_is_edata(engine):
    with pytest.raises(engine.BgzfError) as ex:
        engine.bgzf_decompress(CASES["cut_payload"])
    assert ex.value.code == engine.engine.JDGPU_EDATA and len(ex.value.members) == 1


@pytest.mark.parametrize("align", [16, 1])
def test_device_round_trip_exact_buffers(engine, dev, data, align):
    """every caller buffer of exactly its size, ending at a page end; the
    output 16-byte aligned (decoded in place) or not (gathered)"""
    d = data[:2 * BS + 1232] if align == 16 else data
    comp, offs, back, errs, rc = B.device_round_trip(engine, dev, d, 6, out_align=align)
    assert rc == 0 and back == d and not any(errs)
    assert offs == [r[0] for r in B.walk(comp)[0][:-1]]


def test_bounds_debug_build(engine):
    """the same round trip on the JD_BOUNDS build, loaded as test_bounds.py
    loads it: no access past a caller's buffer"""
    lib = os.path.join(ROOT, "jdeflate_amd", "lib_dbg", "libjdeflate_amd.so")
    if not os.path.exists(lib):
        pytest.fail("JD_BOUNDS library not built (__graft_entry__.build makes it)")
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import jdeflate_amd as J\n"
        "import bgzf_cases as B, test_bgzf_gpu as T\n"
        "d = T.corpus(J)\n"
        "for level, align in ((1, 16), (6, 1), (0, 16)):\n"
        "    H = B.Dev()\n"
        "    comp, offs, back, errs, rc = B.device_round_trip(J, H, d, level, out_align=align)\n"
        "    assert rc == 0 and back == d and not any(errs), (level, align)\n"
        "    assert B.device_index(J, H, comp, 6) == B.walk(comp)\n"
        "    H.free()\n"
        "print('done')\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, JDAMD_LIB=lib)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=240, cwd=ROOT)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "done" in p.stdout, out[-3000:]
    bad = [l for l in out.splitlines() if "JD_BOUNDS" in l]
    assert not bad, "\n".join(bad[:20])
