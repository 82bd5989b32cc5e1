// strand.hip -- both-strand overlaps (SA_OPT_STRANDS = SA_STRANDS_BOTH, gfx950).
//
// The augmented read set is reads 1..2N with read N + i = rc(read i).  The N
// forward reads are uploaded once; revcomp_kernel fills the second half of the
// ASCII buffer on the device, so the unchanged pack kernels yield codes, bad
// positions and locality keys for ids N + 1 .. 2N.  strand_filter then keeps,
// in order, the two flipped classes of the augmented dispatch (DESIGN.md,
// "Both strands").  No reference counterpart: the reference's Overlap.adj is the
// constant 'N' (ObjectStore.scala:121).  Bound: HBM (byte work; no MFMA).
#include "../sa_internal.h"

#include <algorithm>

namespace sa {

// A<->T, C<->G on each byte of x, either case kept; every other byte maps to
// itself.  'A' 0x41 ^ 'T' 0x54 = 0x15, 'C' 0x43 ^ 'G' 0x47 = 0x04: one xor per
// byte, chosen by compares (no table in memory).
__device__ __forceinline__ uint32_t complement4(uint32_t x) {
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t u = (x >> (8 * b)) & 0xDFu;  // upper case
        const uint32_t f = (u == 'A' || u == 'T') ? 0x15u : (u == 'C' || u == 'G') ? 0x04u : 0u;
        m |= f << (8 * b);
    }
    return x ^ m;
}

// One wave per read, one destination dword per lane per iteration (the layout
// of pack_reads_kernel).  Read rd (bytes [b0, b0 + L) of `ascii`) is written
// reversed and complemented to [dst0 + b0, dst0 + b0 + L), dst0 = boff[n], the
// start of the second half.  Destination dword w covers bytes 4w .. 4w + 3;
// its four source bytes are the unaligned dword ending at byte
// s = b0 + (L - 1) - (4w - d0) of the source, read as two aligned dwords and
// funnel-shifted, then byte-reversed.  Read offsets are not dword-aligned, so
// adjacent reads share their first / last dword: a full-dword store is issued
// only for dwords wholly inside this read, the partial head and tail go out as
// byte stores (two waves never write one dword).  Every source byte of a full
// dword lies inside the read; the second aligned dword may reach 3 bytes past
// it, within the buffer (its tail padding), and those bytes are shifted out.
__global__ __launch_bounds__(256) void revcomp_kernel(uint8_t *ascii, const uint64_t *boff, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t dst0 = boff[n];
    for (uint32_t rd = wave; rd < n; rd += nwaves) {
        const uint64_t b0 = boff[rd];
        const int64_t L = (int64_t)(boff[rd + 1] - b0);
        if (L <= 0) continue;
        const uint64_t d0 = dst0 + b0;        // first destination byte
        const uint64_t d1 = d0 + (uint64_t)L; // one past the last
        const uint64_t w0 = d0 >> 2, w1 = (d1 + 3) >> 2;  // destination dwords [w0, w1)
        const uint64_t last = b0 + (uint64_t)L - 1;       // source byte of destination byte d0
        for (uint64_t w = w0 + lane; w < w1; w += 64) {
            const uint64_t a = w << 2;
            if (a >= d0 && a + 4 <= d1) {
                const uint64_t s = last - (a - d0) - 3;  // lowest of the four source bytes, >= b0
                const uint32_t *wp = reinterpret_cast<const uint32_t *>(ascii + (s & ~3ull));
                const uint32_t lo = wp[0], hi = wp[1];
                const uint32_t x = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(s & 3u));
                *reinterpret_cast<uint32_t *>(ascii + a) = complement4(__builtin_bswap32(x));
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint64_t d = a + (uint64_t)t;
                    if (d >= d0 && d < d1) ascii[d] = (uint8_t)complement4((uint32_t)ascii[last - (d - d0)]);
                }
            }
        }
    }
}

hipError_t launch_revcomp(uint8_t *ascii, const uint64_t *boff, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 2048);
    hipLaunchKernelGGL(revcomp_kernel, dim3(blocks), dim3(256), 0, s, ascii, boff, n);
    return hipGetLastError();
}

// ---- strand filter ---------------------------------------------------------
// The augmented dispatch (a, b, count), ids 1-based, lead descending.  Kept:
//   code 2, lead flipped:  a > N >= b and a - N < b   -> (a - N, b)
//   code 1, trail flipped: a <= N < b and a < b - N   -> (a, b - N)
// Dropped: forward x forward (the forward block), rc x rc (its mirror), the
// mirror duplicate of each flipped pair (larger original id on the A side) and
// a read against its own reverse complement.
__device__ __forceinline__ uint32_t strand_code(int32_t a, int32_t b, int32_t N) {
    if (a > N && b <= N && a - N < b) return 2u;
    if (a <= N && b > N && a < b - N) return 1u;
    return 0u;
}

constexpr int SF_THREADS = 256;
constexpr int SF_ROUNDS = 4;  // a block's tile: SF_ROUNDS runs of SF_THREADS consecutive entries
constexpr uint32_t SF_TILE = SF_THREADS * SF_ROUNDS;

// pass 1: kept entries per tile (wave ballots, no atomics)
__global__ __launch_bounds__(SF_THREADS) void strand_count_kernel(const int32_t *lead, const int32_t *trail, uint64_t n,
                                                                  int32_t N, uint32_t *tile_cnt) {
    __shared__ uint32_t wsum[SF_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * SF_TILE;
    uint32_t c = 0;  // wave-uniform
#pragma unroll
    for (int r = 0; r < SF_ROUNDS; ++r) {
        const uint64_t i = base + (uint64_t)r * SF_THREADS + threadIdx.x;
        const bool keep = i < n && strand_code(lead[i], trail[i], N) != 0u;
        c += (uint32_t)__popcll(__ballot(keep));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < SF_THREADS / 64; ++w) t += wsum[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// pass 2: the kept entries of tile t to [tile_off[t], ...), in order: within a
// run of 256 the rank is the wave's prefix (LDS) plus the lane's ballot prefix
__global__ __launch_bounds__(SF_THREADS) void strand_scatter_kernel(const int32_t *lead, const int32_t *trail,
                                                                    const int32_t *count, uint64_t n, int32_t N,
                                                                    const uint32_t *tile_off, int32_t *olead,
                                                                    int32_t *otrail, int32_t *ocount, uint8_t *ocode,
                                                                    int32_t *alead, int32_t *atrail) {
    __shared__ uint32_t wsum[SF_ROUNDS][SF_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * SF_TILE;
    int32_t a[SF_ROUNDS], b[SF_ROUNDS], k[SF_ROUNDS];
    uint32_t code[SF_ROUNDS], pre[SF_ROUNDS];
#pragma unroll
    for (int r = 0; r < SF_ROUNDS; ++r) {
        const uint64_t i = base + (uint64_t)r * SF_THREADS + threadIdx.x;
        code[r] = 0u;
        a[r] = b[r] = k[r] = 0;
        if (i < n) {
            a[r] = lead[i];
            b[r] = trail[i];
            k[r] = count[i];
            code[r] = strand_code(a[r], b[r], N);
        }
        const uint64_t m = __ballot(code[r] != 0u);
        pre[r] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[r][wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t off = tile_off[blockIdx.x];
#pragma unroll
    for (int r = 0; r < SF_ROUNDS; ++r) {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SF_THREADS / 64; ++w) {
            const uint32_t s = wsum[r][w];
            before += (uint32_t)w < wv ? s : 0u;
            all += s;
        }
        if (code[r]) {
            const uint32_t o = off + before + pre[r];
            olead[o] = code[r] == 2u ? a[r] - N : a[r];
            otrail[o] = code[r] == 1u ? b[r] - N : b[r];
            ocount[o] = k[r];
            ocode[o] = (uint8_t)code[r];
            alead[o] = a[r];
            atrail[o] = b[r];
        }
        off += all;
    }
}

uint32_t strand_filter_tiles(uint64_t n) { return (uint32_t)((n + SF_TILE - 1) / SF_TILE); }

// Stable compaction of the augmented dispatch into the flipped block: original
// ids + counts + strand codes, and the augmented ids the aligner takes.  Two
// passes (count, scan, scatter): the order is the input's and the result is the
// same on every run.  tile_cnt: strand_filter_tiles(n) + 1 u32; scan_tmp:
// scan_temp_bytes(strand_filter_tiles(n)); the kept total lands in *total_dev.
// Every output holds up to n entries.
hipError_t launch_strand_filter(const int32_t *lead, const int32_t *trail, const int32_t *count, uint64_t n,
                                uint32_t n_forward, uint32_t *tile_cnt, void *scan_tmp, uint32_t *total_dev,
                                int32_t *olead, int32_t *otrail, int32_t *ocount, uint8_t *ocode, int32_t *alead,
                                int32_t *atrail, hipStream_t s) {
    if (!n) return hipMemsetAsync(total_dev, 0, sizeof(uint32_t), s);
    const uint32_t tiles = strand_filter_tiles(n);
    hipLaunchKernelGGL(strand_count_kernel, dim3(tiles), dim3(SF_THREADS), 0, s, lead, trail, n, (int32_t)n_forward,
                       tile_cnt);
    hipError_t e = exclusive_scan_u32(tile_cnt, tile_cnt, tiles, total_dev, scan_tmp, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(strand_scatter_kernel, dim3(tiles), dim3(SF_THREADS), 0, s, lead, trail, count, n,
                       (int32_t)n_forward, (const uint32_t *)tile_cnt, olead, otrail, ocount, ocode, alead, atrail);
    return hipGetLastError();
}

}  // namespace sa
