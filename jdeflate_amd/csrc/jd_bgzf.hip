/*
 * jd_bgzf.hip -- gfx950 kernels of the BGZF container (jd_bgzf.h): framing
 * of every-block-final deflate output into gzip members, and the index of an
 * arbitrary BGZF buffer with depth logarithmic in the number of members.
 */
#include "jd_device.h"
#include "jd_bgzf.h"
#include "jd_prof.h"

/* ------------------------------------------------------------------------ */
/* framing: one workgroup per member                                         */
/* ------------------------------------------------------------------------ */
#define BZ_T 256u

__constant__ const uint8_t bz_marker[JD_BGZF_EOFLEN] = JD_BGZF_EOF_BYTES;

__device__ static inline uint32_t bz_len(uint64_t n, uint32_t bs, uint32_t b)
{
    const uint64_t o = (uint64_t) b * bs;
    return (uint32_t) (n - o < bs ? n - o : bs);
}

/* payload bytes of block b: its bitstream, or the final stored block that
 * replaces one a member cannot hold (htslib does the same) */
__device__ static inline uint32_t bz_pay(uint32_t csize, uint32_t len)
{
    return csize > JD_BGZF_MAXPAY ? 5u + len : csize;
}

__global__ __launch_bounds__(256) void k_bgzf_size(const uint32_t* __restrict__ csize, uint64_t n,
                                                   uint32_t bs, uint32_t nb,
                                                   uint32_t* __restrict__ msize)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb) msize[b] = bz_pay(csize[b], bz_len(n, bs, b)) + JD_BGZF_FRAME;
}

__global__ __launch_bounds__(BZ_T) void k_bgzf_frame(JdBgzfFrame a)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* oend = a.out + a.outcap;
    (void) oend;
    if (b == a.nblocks) {
        /* the EOF marker after the last member (launched with a.eof only) */
        const uint64_t o = *a.total;
        if (o + JD_BGZF_EOFLEN <= a.outcap && tid < JD_BGZF_EOFLEN) {
            JD_CHECK(a.out + o + tid, 1, oend);
            a.out[o + tid] = bz_marker[tid];
        }
        __syncthreads();
        if (tid == 0) *a.total = o + JD_BGZF_EOFLEN;
        return;
    }
    const uint32_t len = bz_len(a.n, a.bs, b);
    const uint32_t cs = a.csize[b];
    const bool stored = cs > JD_BGZF_MAXPAY;
    const uint32_t pay = bz_pay(cs, len);
    const uint32_t msz = pay + JD_BGZF_FRAME;
    const uint64_t o = a.moff[b];
    if (o + msz > a.outcap) return;
    /* gzip's CRC-32 from k_checksum's register of the block from 0 */
    const uint32_t crc = ~((b == a.lastb ? a.slast : a.sfull) ^ a.ck[3 * (uint64_t) b]);
    /* the bulk source and the member offset of its first byte */
    const uint8_t* src = stored ? a.in + (uint64_t) b * a.bs : a.stage + (uint64_t) b * a.slotcap;
    const uint32_t sbase = stored ? JD_BGZF_HDR + 5u : JD_BGZF_HDR;
    const uint32_t slen = stored ? len : cs;
    const uint32_t* s32 = (const uint32_t*) src;

    auto mbyte = [&](uint32_t k) -> uint32_t {
        if (k < JD_BGZF_HDR) {
            if (k < 16) return bz_marker[k];
            return ((msz - 1) >> (8 * (k - 16))) & 0xffu;
        }
        if (k < JD_BGZF_HDR + pay) {
            if (k >= sbase) return src[k - sbase];
            /* 01 LEN NLEN of the stored block */
            const uint32_t j = k - JD_BGZF_HDR;
            const uint32_t v = len | ((~len & 0xffffu) << 16);
            return j == 0 ? 1u : (v >> (8 * (j - 1))) & 0xffu;
        }
        const uint32_t t = k - JD_BGZF_HDR - pay;
        return ((t < 4 ? crc >> (8 * t) : len >> (8 * (t - 4)))) & 0xffu;
    };

    /* align the destination, then 4-byte stores; in the bulk they are
     * assembled from 4-byte loads of the (aligned) source */
    uint8_t* d = a.out + o;
    const uint32_t head = (uint32_t) ((4 - ((uintptr_t) d & 3)) & 3);
    const uint32_t h = min(head, msz);
    if (tid < h) {
        JD_CHECK(d + tid, 1, oend);
        d[tid] = (uint8_t) mbyte(tid);
    }
    const uint32_t body = (msz - h) / 4;
    uint32_t* d32 = (uint32_t*) (d + h);
    for (uint32_t i = tid; i < body; i += BZ_T) {
        const uint32_t m = h + i * 4;
        uint32_t v;
        if (m >= sbase && m + 8 <= sbase + slen) {
            const uint32_t so = m - sbase;
            v = __builtin_amdgcn_alignbyte(s32[(so >> 2) + 1], s32[so >> 2], so & 3);
        } else {
            v = mbyte(m) | (mbyte(m + 1) << 8) | (mbyte(m + 2) << 16) | (mbyte(m + 3) << 24);
        }
        JD_CHECK(d32 + i, 4, oend);
        d32[i] = v;
    }
    const uint32_t tail0 = h + body * 4;
    if (tid < msz - tail0) {
        JD_CHECK(d + tail0 + tid, 1, oend);
        d[tail0 + tid] = (uint8_t) mbyte(tail0 + tid);
    }
}

extern "C" int jdk_bgzf_frame_launch(const JdBgzfFrame* F)
{
    hipStream_t st = (hipStream_t) F->stream;
    const uint32_t nb = F->nblocks;
    if (nb) {
        JDPROF_RUN(JDK_BGZF_FRAME, st, (k_bgzf_size<<<(nb + 255) / 256, 256, 0, st>>>(F->csize, F->n, F->bs, nb, F->msize)));
        if (jdk_scan_launch(F->msize, nb, F->moff, F->total, F->base, st)) return -1;
    }
    if (nb + (F->eof ? 1u : 0u))
        JDPROF_RUN(JDK_BGZF_FRAME, st, (k_bgzf_frame<<<nb + (F->eof ? 1u : 0u), BZ_T, 0, st>>>(*F)));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* ------------------------------------------------------------------------ */
/* index                                                                     */
/*
 * k_bgzf_scan tests every byte position for a valid member header; the
 * candidates (false ones inside payloads included) are compacted in position
 * order with each one's successor position.  k_bgzf_link resolves the
 * successor to a candidate, END (the buffer's end) or INVALID (not a
 * candidate); both are fixed points.  k_bgzf_double squares the successor
 * map (J <- J o J) while it adds up the hops to the fixed point (D) and marks
 * what candidate 0 reaches; after ceil(log2) rounds the members are the
 * marked nodes, and member i's ordinal is D[0] - D[i].  k_bgzf_emit scatters
 * them.  The result equals jd_bgzf_walk's.
 */
/* ------------------------------------------------------------------------ */
#define BZ_PER 16u
#define BZ_WG  (BZ_T * BZ_PER)

extern "C" uint64_t jdk_bgzf_groups(uint64_t n) { return (n + BZ_WG - 1) / BZ_WG; }

__device__ static inline uint32_t bz_le16(const uint8_t* p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }

/* jd_bgzf_walk.c bgzf_header; the magic at off is already known */
__device__ static bool bz_header(const uint8_t* p, uint64_t n, uint64_t off, uint32_t* xlen, uint32_t* bsize)
{
    if (n - off < 12) return false;
    const uint32_t xl = bz_le16(p + off + 10);
    if (xl < 6 || n - off - 12 < xl) return false;
    uint64_t q = off + 12;
    const uint64_t end = q + xl;
    while (end - q >= 4) {
        const uint32_t slen = bz_le16(p + q + 2);
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2) {
            if (end - q < 6) return false;
            const uint32_t bs = bz_le16(p + q + 4);
            if (bs + 1 < xl + 20 || n - off < (uint64_t) bs + 1) return false;
            *xlen = xl;
            *bsize = bs;
            return true;
        }
        if (end - q - 4 < slen) return false;
        q += 4 + slen;
    }
    return false;
}

/* WRITE = false: wcnt[g] = candidates in group g's BZ_WG positions.
 * WRITE = true: they are written at woff[g] in position order. */
template <bool WRITE>
__global__ __launch_bounds__(BZ_T) void k_bgzf_scan(const uint8_t* __restrict__ in, uint64_t n,
                                                    uint32_t* __restrict__ wcnt,
                                                    const uint64_t* __restrict__ woff, uint32_t cap,
                                                    uint64_t* __restrict__ cpos,
                                                    uint64_t* __restrict__ cnext,
                                                    uint32_t* __restrict__ cxl)
{
    __shared__ uint32_t part[BZ_T];
    const uint32_t tid = threadIdx.x, g = blockIdx.x;
    if (WRITE && wcnt[g] == 0) return;
    const uint64_t p0 = ((uint64_t) g * BZ_T + tid) * BZ_PER;
    /* the thread's 16 positions need bytes [p0, p0 + 19) */
    uint32_t w[5] = {0, 0, 0, 0, 0};
    if (p0 + 20 <= n) {
        const uint4 v = *(const uint4*) (in + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        w[4] = *(const uint32_t*) (in + p0 + 16);
    } else {
        for (uint32_t k = 0; k < 20 && p0 + k < n; k++) w[k >> 2] |= (uint32_t) in[p0 + k] << (8 * (k & 3));
    }
    uint32_t fk[4], fx[4], nf = 0;
#pragma unroll
    for (uint32_t k = 0; k < BZ_PER; k++) {
        const uint32_t x = (k & 3) ? __builtin_amdgcn_alignbyte(w[(k >> 2) + 1], w[k >> 2], k & 3) : w[k >> 2];
        if (x == 0x04088b1fu && p0 + k + 4 <= n) {
            uint32_t xl, bs;
            if (bz_header(in, n, p0 + k, &xl, &bs) && nf < 4) {
                fk[nf] = k;
                fx[nf] = xl | (bs << 16);
                nf++;
            }
        }
    }
    part[tid] = nf;
    __syncthreads();
    for (uint32_t o = 1; o < BZ_T; o <<= 1) {
        const uint32_t x = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    if (!WRITE) {
        if (tid == BZ_T - 1) wcnt[g] = part[tid];
        return;
    }
    const uint64_t base = woff[g] + part[tid] - nf;
    for (uint32_t j = 0; j < nf; j++) {
        const uint64_t i = base + j;
        if (i >= cap) break;
        cpos[i] = p0 + fk[j];
        cnext[i] = p0 + fk[j] + (fx[j] >> 16) + 1;
        cxl[i] = fx[j];
    }
}

/* node ids: candidates 0 .. C-1, END = C, INVALID = C + 1 */
__global__ __launch_bounds__(256) void k_bgzf_link(const uint64_t* __restrict__ cpos,
                                                   const uint64_t* __restrict__ cnext,
                                                   const uint64_t* __restrict__ ctotal, uint32_t cap,
                                                   uint64_t n, uint32_t* __restrict__ J,
                                                   uint32_t* __restrict__ D, uint32_t* __restrict__ mark)
{
    const uint64_t ct = *ctotal;
    const uint32_t C = ct > cap ? 0u : (uint32_t) ct;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C + 2) return;
    if (i >= C) {
        J[i] = i;
        D[i] = 0;
        mark[i] = 0;
        return;
    }
    const uint64_t q = cnext[i];
    uint32_t j = C + 1;
    if (q == n) {
        j = C;
    } else {
        /* candidates are sorted by position, and q > cpos[i] */
        uint32_t lo = i + 1, hi = C;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cpos[mid] < q) lo = mid + 1; else hi = mid;
        }
        if (lo < C && cpos[lo] == q) j = lo;
    }
    J[i] = j;
    D[i] = 1;
    mark[i] = (i == 0 && cpos[0] == 0) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_bgzf_double(const uint32_t* __restrict__ Ji,
                                                     const uint32_t* __restrict__ Di,
                                                     uint32_t* __restrict__ Jo, uint32_t* __restrict__ Do,
                                                     uint32_t* mark, const uint64_t* __restrict__ ctotal,
                                                     uint32_t cap)
{
    const uint64_t ct = *ctotal;
    const uint32_t C = ct > cap ? 0u : (uint32_t) ct;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C + 2) return;
    const uint32_t j = Ji[i];
    Jo[i] = Ji[j];
    Do[i] = Di[i] + Di[j];
    /* what candidate 0 reaches in fewer than 2^k hops reaches j in fewer than
     * 2^(k+1); a mark set during this round only adds a node it reaches too */
    if (j < C && mark[i]) mark[j] = 1;
}

__global__ __launch_bounds__(256) void k_bgzf_emit(JdBgzfIndex x, const uint32_t* __restrict__ J,
                                                   const uint32_t* __restrict__ D,
                                                   const uint32_t* __restrict__ mark)
{
    const uint64_t ct = *x.ctotal;
    const bool over = ct > x.candcap;
    const uint32_t C = over ? 0u : (uint32_t) ct;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool rooted = C && x.cpos[0] == 0;
    const uint32_t M = rooted ? D[0] : 0u;
    if (i == 0) {
        int32_t s = 0;
        uint32_t nb = M;
        if (over) { s = JD_BGZF_ECAP; nb = 0; }
        else if (M > x.maxblocks) { s = JD_BGZF_ECAP; nb = x.maxblocks; }
        else if (!rooted) s = x.n ? JD_BGZF_EDATA : 0;
        else if (J[0] != C) s = JD_BGZF_EDATA;
        *x.status = s;
        *x.nblocks = nb;
    }
    if (i >= C || !rooted || !mark[i]) return;
    const uint32_t ord = M - D[i];
    if (ord >= x.maxblocks) return;
    const uint64_t p = x.cpos[i];
    const uint32_t xl = x.cxl[i] & 0xffffu, bs = x.cxl[i] >> 16;
    const uint8_t* t = x.in + p + bs + 1 - 8;
    x.moff[ord] = p;
    x.poff[ord] = p + 12 + xl;
    x.psize[ord] = bs + 1 - xl - 20;
    x.crc[ord] = (uint32_t) t[0] | ((uint32_t) t[1] << 8) | ((uint32_t) t[2] << 16) | ((uint32_t) t[3] << 24);
    x.isize[ord] = (uint32_t) t[4] | ((uint32_t) t[5] << 8) | ((uint32_t) t[6] << 16) | ((uint32_t) t[7] << 24);
    /* the chain's last member (x.eof was cleared before the launch) */
    if (D[i] == 1 && J[i] == C && M <= x.maxblocks && bs + 1 == JD_BGZF_EOFLEN) {
        bool same = true;
        for (uint32_t k = 0; k < JD_BGZF_EOFLEN; k++) same = same && x.in[p + k] == bz_marker[k];
        if (same) *x.eof = 1;
    }
}

extern "C" int jdk_bgzf_index_launch(const JdBgzfIndex* X)
{
    hipStream_t st = (hipStream_t) X->stream;
    const uint64_t ng = jdk_bgzf_groups(X->n);
    if (ng > 0xffffffffull) return -1;
    const uint32_t cap = X->candcap;
    uint32_t* J0 = X->jd;
    uint32_t* D0 = J0 + (cap + 2);
    uint32_t* J1 = D0 + (cap + 2);
    uint32_t* D1 = J1 + (cap + 2);
    uint32_t* mark = D1 + (cap + 2);
    if (hipMemsetAsync(X->eof, 0, 4, st) != hipSuccess || hipMemsetAsync(X->ctotal, 0, 8, st) != hipSuccess)
        return -1;
    if (ng) {
        JDPROF_RUN(JDK_BGZF_INDEX, st, (k_bgzf_scan<false><<<(uint32_t) ng, BZ_T, 0, st>>>(X->in, X->n, X->wcnt, nullptr, cap,
                                                                                   nullptr, nullptr, nullptr)));
        if (jdk_scan_launch(X->wcnt, (uint32_t) ng, X->woff, X->ctotal, nullptr, st)) return -1;
        JDPROF_RUN(JDK_BGZF_INDEX, st, (k_bgzf_scan<true><<<(uint32_t) ng, BZ_T, 0, st>>>(X->in, X->n, X->wcnt, X->woff, cap,
                                                                                  X->cpos, X->cnext, X->cxl)));
    }
    const uint32_t grid = (cap + 2 + 255) / 256;
    JDPROF_RUN(JDK_BGZF_INDEX, st, (k_bgzf_link<<<grid, 256, 0, st>>>(X->cpos, X->cnext, X->ctotal, cap, X->n, J0, D0, mark)));
    /* 2^rounds >= cap + 2 nodes: every node stands on a fixed point */
    uint32_t rounds = 1;
    while ((1ull << rounds) < (uint64_t) cap + 2) rounds++;
    for (uint32_t r = 0; r < rounds; r++) {
        JDPROF_RUN(JDK_BGZF_INDEX, st, (k_bgzf_double<<<grid, 256, 0, st>>>(J0, D0, J1, D1, mark, X->ctotal, cap)));
        uint32_t* t = J0; J0 = J1; J1 = t;
        t = D0; D0 = D1; D1 = t;
    }
    JDPROF_RUN(JDK_BGZF_INDEX, st, (k_bgzf_emit<<<grid, 256, 0, st>>>(*X, J0, D0, mark)));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
