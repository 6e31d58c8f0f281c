/*
 * jd_bgzf_walk.c -- the serial walk over the members of a BGZF buffer
 * (jd_bgzf.h).  Plain C, no device: the host-buffer entry points use it, and
 * the device index (jd_bgzf.hip) is defined to give the same result.
 */
#include <string.h>

#include "jd_bgzf.h"

static uint32_t le16(const uint8_t* p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }

static uint32_t le32(const uint8_t* p)
{
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}

/* 1 when a valid member header stands at off; its XLEN and BSIZE */
static int bgzf_header(const uint8_t* p, uint64_t n, uint64_t off, uint32_t* xlen, uint32_t* bsize)
{
    uint64_t q, end;
    uint32_t xl;
    if (off > n || n - off < 12) return 0;
    if (p[off] != 0x1f || p[off + 1] != 0x8b || p[off + 2] != 0x08 || p[off + 3] != 0x04) return 0;
    xl = le16(p + off + 10);
    if (xl < 6 || n - off - 12 < xl) return 0;
    q = off + 12;
    end = q + xl;
    while (end - q >= 4) {
        const uint32_t slen = le16(p + q + 2);
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2) {
            uint32_t bs;
            if (end - q < 6) return 0;
            bs = le16(p + q + 4);
            if (bs + 1 < xl + 20 || n - off < (uint64_t) bs + 1) return 0;
            *xlen = xl;
            *bsize = bs;
            return 1;
        }
        if (end - q - 4 < slen) return 0;
        q += 4 + slen;
    }
    return 0;
}

int jd_bgzf_walk(const uint8_t* p, uint64_t n, uint32_t maxblocks, uint64_t* moff,
                 uint64_t* poff, uint32_t* psize, uint32_t* isize, uint32_t* crc,
                 uint32_t* nblocks, uint32_t* eof)
{
    static const uint8_t marker[JD_BGZF_EOFLEN] = JD_BGZF_EOF_BYTES;
    uint64_t off = 0;
    uint32_t k = 0, last = 0;
    int r = 0;
    while (off < n) {
        uint32_t xl, bs;
        if (!bgzf_header(p, n, off, &xl, &bs)) { r = JD_BGZF_EDATA; break; }
        if (k == maxblocks) { r = JD_BGZF_ECAP; break; }
        if (moff) moff[k] = off;
        if (poff) poff[k] = off + 12 + xl;
        if (psize) psize[k] = bs + 1 - xl - 20;
        if (crc) crc[k] = le32(p + off + bs + 1 - 8);
        if (isize) isize[k] = le32(p + off + bs + 1 - 4);
        last = bs + 1 == JD_BGZF_EOFLEN && memcmp(p + off, marker, JD_BGZF_EOFLEN) == 0;
        k++;
        off += (uint64_t) bs + 1;
    }
    if (nblocks) *nblocks = k;
    if (eof) *eof = (r == 0 && k) ? last : 0;
    return r;
}
