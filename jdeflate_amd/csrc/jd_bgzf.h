/*
 * jd_bgzf.h -- BGZF (blocked gzip: htslib, bgzip, BAM, tabix) container
 * support shared by the host walk (jd_bgzf_walk.c), the kernels
 * (jd_bgzf.hip) and the engine (internal; not installed).
 *
 * A BGZF file is a series of gzip members of at most 65536 bytes:
 *     1f 8b 08 04  MTIME(4)  XFL OS  XLEN(le16)  extra field (XLEN bytes)
 *     deflate payload  CRC32(le32)  ISIZE(le32)
 * whose extra field holds a subfield 'B' 'C' of length 2: BSIZE (le16) =
 * member size - 1.  The file ends with a fixed empty member of 28 bytes.
 */
#ifndef JD_BGZF_H
#define JD_BGZF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JD_BGZF_MAXBS    65280u   /* input bytes per member (htslib's 0xff00)   */
#define JD_BGZF_MAXPAY   65510u   /* payload bytes: 65536 - 18 - 8              */
#define JD_BGZF_HDR      18u      /* header with the one BC subfield            */
#define JD_BGZF_FRAME    26u      /* header + trailer                           */
#define JD_BGZF_EOFLEN   28u
#define JD_BGZF_EOF_BYTES                                                          \
    { 0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, \
      0x43, 0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, \
      0x00, 0x00 }

/* results of the walk / the device index (the JDGPU_E* values of jdgpu.h) */
#define JD_BGZF_ECAP  (-4)
#define JD_BGZF_EDATA (-5)

/*
 * The serial walk over the members of p[0, n) from offset 0: the statement
 * of the format the device index is defined to equal.  Member k is valid when
 * 1f 8b 08 is present, FLG is exactly 0x04, XLEN >= 6, the walk over the extra
 * field's subfields finds a 'B','C' subfield of length 2, BSIZE + 1 >=
 * XLEN + 20 and the member ends within the buffer.  For every valid member up
 * to maxblocks the arrays (each may be NULL) receive its offset, its payload
 * offset and size and the trailer's ISIZE and CRC; *nblocks the number of
 * valid members from offset 0, *eof whether the last one is the EOF marker.
 * Returns 0 when the chain ends exactly at n, JD_BGZF_EDATA when it stops on
 * an invalid member (the last good one is member *nblocks - 1), JD_BGZF_ECAP
 * when there are more than maxblocks members (*nblocks = maxblocks then).
 */
int jd_bgzf_walk(const uint8_t* p, uint64_t n, uint32_t maxblocks, uint64_t* moff,
                 uint64_t* poff, uint32_t* psize, uint32_t* isize, uint32_t* crc,
                 uint32_t* nblocks, uint32_t* eof);

/* ---- jd_bgzf.hip (all pointers device) --------------------------------- */

/* The members of one deflate launch chunk: block b's payload is its stage
 * slot (csize[b] bytes) or, when that exceeds JD_BGZF_MAXPAY, the block as
 * one final stored block read from `in`.  Member sizes are scanned into
 * moff (offsets from *base, or 0) and *total; with `eof` the marker follows
 * the last member and *total counts it. */
typedef struct {
    const uint8_t* in;      /* the chunk's input, 16-byte aligned          */
    uint64_t n;             /* its bytes                                   */
    uint32_t bs, nblocks;   /* nblocks may be 0 (the marker alone)         */
    const uint8_t* stage;
    uint32_t slotcap;
    const uint32_t* csize;
    const uint32_t* ck;     /* k_checksum's triples of the blocks          */
    uint32_t sfull, slast;  /* the register 0xFFFFFFFF advanced over bs
                               bytes, and over the last block's            */
    uint32_t lastb;         /* the input's last block in this chunk, or ~0 */
    uint32_t eof;
    uint32_t* msize;        /* scratch: nblocks                            */
    uint64_t* moff;         /* nblocks                                     */
    uint64_t* total;
    const uint64_t* base;
    uint8_t* out;
    uint64_t outcap;
    void* stream;
} JdBgzfFrame;

int jdk_bgzf_frame_launch(const JdBgzfFrame* F);

/* Index of the members of in[0, n) (16-byte aligned), equal to jd_bgzf_walk's:
 * status[0] = 0 / JD_BGZF_EDATA / JD_BGZF_ECAP.  Scratch: candcap candidates. */
typedef struct {
    const uint8_t* in;
    uint64_t n;
    uint32_t maxblocks, candcap;
    uint32_t* wcnt;         /* jdk_bgzf_groups(n) + 1                      */
    uint64_t* woff;         /* jdk_bgzf_groups(n) + 1                      */
    uint64_t* ctotal;       /* 1                                           */
    uint64_t* cpos;         /* candcap                                     */
    uint64_t* cnext;        /* candcap                                     */
    uint32_t* cxl;          /* candcap                                     */
    uint32_t* jd;           /* 5 * (candcap + 2): J, D ping-pong, marks    */
    uint64_t* moff;         /* maxblocks each                              */
    uint64_t* poff;
    uint32_t* psize;
    uint32_t* isize;
    uint32_t* crc;
    uint32_t* nblocks;      /* 1                                           */
    uint32_t* eof;          /* 1                                           */
    int32_t* status;        /* 1                                           */
    void* stream;
} JdBgzfIndex;

uint64_t jdk_bgzf_groups(uint64_t n);
int jdk_bgzf_index_launch(const JdBgzfIndex* X);

/* jd_check.hip: member b = in + b * stride, usize[b] bytes decoded.  Where
 * err[b] is 0 it becomes esize when usize[b] != isize[b], else ecrc when the
 * gzip CRC-32 of the bytes differs from crc[b]. */
int jdk_checksum_members_launch(const uint8_t* in, uint32_t stride, uint32_t nblocks,
                                const uint32_t* usize, const uint32_t* isize,
                                const uint32_t* crc, const uint32_t* shiftm, int32_t* err,
                                int32_t esize, int32_t ecrc, void* stream);

/* jd_deflate.hip: k_scan and k_compact on their own */
int jdk_scan_launch(const uint32_t* sz, uint32_t nb, uint64_t* off, uint64_t* total,
                    const uint64_t* base, void* stream);
int jdk_compact_launch(const uint8_t* stage, uint32_t slotcap, const uint32_t* sz,
                       const uint64_t* off, uint32_t nb, uint8_t* out, uint64_t outcap,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
