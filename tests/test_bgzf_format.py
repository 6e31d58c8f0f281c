"""The BGZF member walk (jd_bgzf_walk, behind jdgpu_bgzf_index) against the
test's own pure-Python walk, on files made by a pure-Python writer.  No GPU.
The same files go through a stand-alone program built from jd_bgzf_walk.c
with AddressSanitizer and UBSan, every file in a heap block of exactly its
size."""
import os
import subprocess

import pytest

import bgzf_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jdeflate_amd", "csrc")
CASES = B.cases()


@pytest.fixture(scope="module")
def J(built_lib):
    import jdeflate_amd as J
    J.load_library()
    return J


def host_index(J, buf, maxblocks=None):
    try:
        rows, eof = J.bgzf_index(buf, maxblocks=maxblocks, full=True)
        return rows, eof, 0
    except J.BgzfError as ex:
        return ex.members, False, ex.code


@pytest.mark.parametrize("name", sorted(CASES))
def test_index_equals_python_walk(J, name):
    buf = CASES[name]
    assert host_index(J, buf) == B.walk(buf)


def test_cases_are_what_they_claim():
    """the files exercise what their names say (from the Python walk alone)"""
    w = {k: B.walk(v) for k, v in CASES.items()}
    datas, ms = B.variable_members()
    assert [r[3] for r in w["variable_eof"][0]] == [1, 4097, 65280, 65536, 0]
    assert w["variable_eof"][1:] == (True, 0) and w["variable_noeof"][1:] == (False, 0)
    assert [r[3] for r in w["empty_mid"][0]] == [4097, 0, 1, 0]
    assert [r[1] - r[0] for r in w["extra_before_bc"][0]] == [25, 28, 18]
    for name, good in (("cut_header", 2), ("cut_payload", 1), ("cut_trailer", 1), ("bsize_past_end", 1)):
        rows, eof, st = w[name]
        assert st == B.EDATA and len(rows) == good and not eof, name
    assert w["cut_header"][0][-1][0] == len(ms[0])          # the last good member's offset
    # a whole valid member inside a stored payload is no member of the file
    rows, eof, st = w["fake_in_stored"]
    assert st == 0 and eof and len(rows) == 3
    inner = CASES["fake_in_stored"].find(b"\x1f\x8b\x08\x04", rows[1][0] + 4)
    assert rows[1][1] < inner < rows[2][0] and B.walk(CASES["fake_in_stored"][inner:])[0]
    assert len(w["minimal_300"][0]) == 300 and len(CASES["minimal_300"]) < 65536
    assert w["only_eof"] == ([(0, 18, 2, 0, 0)], True, 0)
    assert w["empty"] == ([], False, 0) and w["garbage"] == ([], False, B.EDATA)


def test_capacity(J):
    buf = CASES["variable_eof"]
    rows, eof, st = host_index(J, buf, maxblocks=4)
    assert st == B.ECAP and rows == B.walk(buf)[0][:4] and not eof
    assert host_index(J, buf, maxblocks=5) == B.walk(buf)


def test_python_api_shape(J):
    buf = CASES["variable_eof"]
    assert J.bgzf_index(buf) == [(r[0], r[2], r[3], r[4]) for r in B.walk(buf)[0]]
    assert J.bgzf_bound(0) == 28 and J.bgzf_bound(1, 65296) == 0 and J.bgzf_bound(1, 100) == 0
    assert J.bgzf_bound(65280) == 65536 + 28 and J.BGZF_EOF == B.EOF


MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include "jd_bgzf.h"
int main(int argc, char** argv)
{
    int a;
    for (a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        long n;
        uint8_t* p;
        uint32_t nb = 0, eof = 0, k, cap;
        int r;
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        n = ftell(f);
        fseek(f, 0, SEEK_SET);
        p = malloc(n ? n : 1);                 /* exactly the file: ASan guards both ends */
        if (n && fread(p, 1, n, f) != (size_t) n) return 2;
        fclose(f);
        r = jd_bgzf_walk(p, n, 0xffffffffu, NULL, NULL, NULL, NULL, NULL, &nb, &eof);
        printf("%d %u %u", r, nb, eof);
        cap = nb ? nb : 1;
        {
            uint64_t* mo = malloc(cap * 8), * po = malloc(cap * 8);
            uint32_t* ps = malloc(cap * 4), * is = malloc(cap * 4), * cr = malloc(cap * 4);
            jd_bgzf_walk(p, n, nb, mo, po, ps, is, cr, &k, NULL);
            if (k != nb) return 3;
            for (k = 0; k < nb; k++)
                printf(" %llu:%llu:%u:%u:%u", (unsigned long long) mo[k], (unsigned long long) po[k],
                       ps[k], is[k], cr[k]);
            free(mo); free(po); free(ps); free(is); free(cr);
        }
        printf("\n");
        free(p);
    }
    return 0;
}
'''


def test_walk_under_sanitizers(tmp_path):
    """jd_bgzf_walk.c alone with a main of its own, -fsanitize=address,undefined,
    over every file: clean, and the same index again"""
    (tmp_path / "main.c").write_text(MAIN)
    exe = tmp_path / "walk_san"
    subprocess.run(["gcc", "-std=c99", "-g", "-O1", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "main.c"),
                    os.path.join(CSRC, "jd_bgzf_walk.c"), "-o", str(exe)], check=True)
    names = sorted(CASES)
    paths = []
    for k in names:
        p = tmp_path / (k + ".bgzf")
        p.write_bytes(CASES[k])
        paths.append(str(p))
    r = subprocess.run([str(exe)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    for k, line in zip(names, lines):
        f = line.split()
        rows, eof, st = B.walk(CASES[k])
        assert (int(f[0]), int(f[1]), int(f[2])) == (st, len(rows), int(eof)), k
        assert [tuple(int(x) for x in t.split(":")) for t in f[3:]] == rows, k
