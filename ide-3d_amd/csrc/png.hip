// png.hip — the zlib stream of a PNG file from uint8 frames on the device: the compression half of
// `save_image(imgs, 'seed0000.png', ...)` (gen_images.py:115-116).  training/png.py states the stream in integers (row filters, the
// token rule, code lengths with their tie-breaking, the header's run-length coding, the stored fallback); every kernel here reproduces
// those integers, so device and host files are equal byte for byte.  Integer arithmetic only.
//
//   filter    one workgroup per row: the five PNG filters on 16 bytes per lane, the adaptive choice (sum of min(v, 256 - v), lowest type
//             on a tie), [type | filtered row] into the frame's filtered stream (frames 16-byte aligned in the workspace)
//   deflate   one workgroup per segment of `segment_bytes` filtered bytes: Adler-32 partial sums, run tokens (literal + distance-1
//             matches), histogram, length-limited Huffman lengths, the dynamic header, bit packing in LDS; or one stored block.  The
//             segment's bytes go to its own slot of the workspace (at most n + 5 bytes)
//   scan      segment_positions_kernel (block_scan.h): the position of every segment in `out`, `offsets`
//   compact   one workgroup per segment: slot -> out; the frame's first segment also writes 78 01 and the combined Adler-32
//
// LDS atomics (integer add / or) only where the result does not depend on order: two runs are bit-equal.
#include "block_scan.h"

namespace ide3d {

constexpr int kPngThreads = 256;
constexpr int kPngDeflateThreads = 1024;            // 32 bytes of a 32 KiB segment per thread: its walks are the segment's latency
constexpr int kPngTile = kPngThreads * 16;          // source bytes of a row per filter pass
constexpr int kPngSyms = 286;                       // literal / length alphabet
constexpr int kPngClSyms = 19;
constexpr int kPngMinSeg = 1024, kPngMaxSeg = 32768;
constexpr int kPngSlotPad = 32;                     // slot = segment_bytes + 32: n + 5 rounded up to 16, and one 16-byte group of read-ahead
constexpr unsigned kAdler = 65521u;

struct PngShape {
    int N, H, W, C;
    int row;             // W * C
    int seg, S;          // segment bytes, segments per frame
    int64_t F, Fpad;     // filtered bytes per frame, rounded up to 16
    int64_t T;           // N * S
};

struct PngSegInfo { unsigned size, a, b, pad; };
__constant__ uint8_t kPngClOrder[kPngClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};          // RFC 1951 3.2.7

static bool png_shape(int32_t N, int32_t H, int32_t W, int32_t C, int32_t seg, PngShape& s) {
    if (N < 1 || H < 1 || W < 1 || (C != 1 && C != 3)) return false;
    if (seg < kPngMinSeg || seg > kPngMaxSeg || (seg & (seg - 1))) return false;
    const int64_t row = (int64_t)W * C, F = (int64_t)H * (row + 1);
    if (row >= (1ll << 31) - 1 || F >= (1ll << 31) || (int64_t)N * H >= (1ll << 31)) return false;
    s.N = N; s.H = H; s.W = W; s.C = C; s.row = (int)row; s.seg = seg;
    s.F = F; s.Fpad = (F + 15) / 16 * 16;
    s.S = (int)((F + seg - 1) / seg);
    s.T = (int64_t)N * s.S;
    // everything the kernels index stays below 2^31
    if ((int64_t)N * s.Fpad >= (1ll << 31) || s.T * (seg + kPngSlotPad) >= (1ll << 31)) return false;
    return true;
}
static int64_t png_worst_case(const PngShape& s) { return (int64_t)s.N * (s.F + 5ll * s.S + 6); }
static int64_t png_slots_offset(const PngShape& s) { return (int64_t)s.N * s.Fpad; }
static int64_t png_info_offset(const PngShape& s) { return png_slots_offset(s) + s.T * (s.seg + kPngSlotPad); }
static int64_t png_pos_offset(const PngShape& s) { return png_info_offset(s) + s.T * 16; }
static int64_t png_workspace(const PngShape& s) { return png_pos_offset(s) + (s.T * 8 + 15) / 16 * 16; }

// ---- stage a: rows ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int png_filtered(int t, int x, int a, int b, int c) {
    const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
    return (x - pred) & 255;
}

// Bytes [x - 3, x + 16) of a row of `len` bytes into v[19] (0 outside the row, and everywhere when the row does not exist).  `wide`: the
// row starts on a 16-byte boundary and x is a multiple of 16, so a whole group is one 16-byte load and its left neighbours one 4-byte load.
__device__ __forceinline__ void png_load_group(const uint8_t* __restrict__ rowp, bool exists, bool wide, int x, int len, uint8_t* v) {
#pragma unroll
    for (int j = 0; j < 19; ++j) v[j] = 0;
    if (!exists || x >= len) return;
    if (wide && x + 16 <= len) {
        const uint4 q = *reinterpret_cast<const uint4*>(rowp + x);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) v[3 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        if (x >= 4) {
            const unsigned l = *reinterpret_cast<const unsigned*>(rowp + x - 4);
            v[0] = (uint8_t)(l >> 8); v[1] = (uint8_t)(l >> 16); v[2] = (uint8_t)(l >> 24);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 19; ++j) {
            const int p = x - 3 + j;
            if (p >= 0 && p < len) v[j] = rowp[p];
        }
    }
}

template <int bpp>
__global__ void __launch_bounds__(kPngThreads)
png_filter_kernel(const uint8_t* __restrict__ frames, const PngShape s, int mode, int wide, uint8_t* __restrict__ filtered) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kPngTile + 32];
    __shared__ unsigned long long s_cost[5];          // a lane's own sums fit 32 bits (row < 2^31 bytes over 256 lanes), the row's may not
    const int r = (int)blockIdx.x;                        // row of the batch: scalar
    if (r >= s.N * s.H) return;
    const int f = r / s.H, y = r - f * s.H;
    const int len = s.row;
    const uint8_t* const cur = frames + (int64_t)r * len;
    const uint8_t* const up = cur - len;                  // read only when y > 0
    uint8_t* const dst = filtered + (int64_t)f * s.Fpad + (int64_t)y * (len + 1);
    int type = mode;
    if (mode == 5) {
        if (threadIdx.x < 5) s_cost[threadIdx.x] = 0;
        __syncthreads();
        unsigned cost[5] = {0, 0, 0, 0, 0};
        for (int x = (int)threadIdx.x * 16; x < len; x += kPngTile) {
            uint8_t vc[19], vu[19];
            png_load_group(cur, true, wide != 0, x, len, vc);
            png_load_group(up, y > 0, wide != 0, x, len, vu);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (x + j < len) {
                    const int xx = vc[3 + j], a = vc[3 + j - bpp], b = vu[3 + j], c = vu[3 + j - bpp];
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        const int v = png_filtered(t, xx, a, b, c);
                        cost[t] += (unsigned)min(v, 256 - v);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            unsigned long long v = cost[t];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if ((threadIdx.x & 63) == 0) atomicAdd(&s_cost[t], v);          // integer sum: order does not matter
        }
        __syncthreads();
        type = 0;
        unsigned long long best = s_cost[0];
#pragma unroll
        for (int t = 1; t < 5; ++t) if (s_cost[t] < best) { best = s_cost[t]; type = t; }
    }
    if (threadIdx.x == 0) dst[0] = (uint8_t)type;
    for (int x0 = 0; x0 < len; x0 += kPngTile) {
        const int tl = min(kPngTile, len - x0);                             // source bytes of this tile
        uint8_t* const d0 = dst + 1 + x0;                                   // where they go
        const int mis = (int)(reinterpret_cast<uintptr_t>(d0) & 15);         // s_out[i] <-> address (d0 - mis) + i
        const int x = x0 + (int)threadIdx.x * 16;
        if (x < len) {
            uint8_t vc[19], vu[19];
            png_load_group(cur, true, wide != 0, x, len, vc);
            png_load_group(up, y > 0, wide != 0, x, len, vu);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (x + j < len)
                    s_out[mis + (x - x0) + j] = (uint8_t)png_filtered(type, vc[3 + j], vc[3 + j - bpp], vu[3 + j], vu[3 + j - bpp]);
        }
        __syncthreads();
        const int groups = (mis + tl + 15) >> 4;
        for (int g = (int)threadIdx.x; g < groups; g += kPngThreads) {
            const int lo = g * 16, hi = lo + 16;
            if (lo >= mis && hi <= mis + tl) {
                *reinterpret_cast<uint4*>(d0 - mis + lo) = *reinterpret_cast<const uint4*>(s_out + lo);
            } else {
                for (int i = max(lo, mis); i < min(hi, mis + tl); ++i) (d0 - mis)[i] = s_out[i];
            }
        }
        __syncthreads();
    }
}

// ---- stage b: segments ------------------------------------------------------------------------------------------------------------

// Length 3..258 -> literal/length symbol, number of extra bits and their value (RFC 1951 3.2.5).
__device__ __forceinline__ void png_length_code(int length, int& sym, int& ebits, int& evalue) {
    const int l = length - 3;
    if (length == 258) { sym = 285; ebits = 0; evalue = 0; }
    else if (l < 8) { sym = 257 + l; ebits = 0; evalue = 0; }
    else {
        ebits = 29 - __clz(l);                       // floor(log2 l) - 2
        sym = 257 + 4 * (ebits + 1) + ((l >> ebits) & 3);
        evalue = l & ((1 << ebits) - 1);
    }
}

struct PngHuffScratch {
    unsigned w[2 * kPngSyms];            // node weights: leaves in (count, symbol) order, then internal nodes in creation order
    unsigned short parent[2 * kPngSyms];
    unsigned short depth[2 * kPngSyms];
    unsigned short rank[kPngSyms + 2];   // symbol -> position among the used symbols
    unsigned num[kPngSyms + 2];          // leaves per depth; after the limiter: codes per length
    unsigned cum[17], next[17];
    int n;
};

// Code lengths (<= limit) and bit-reversed canonical codes of `nsym` symbols from their counts: training/png.py::code_lengths /
// canonical_codes.  Every thread of the workgroup calls it; freq is read-only, lens / codes are complete after the call.
__device__ void png_huffman(const unsigned* freq, int nsym, int limit, uint8_t* lens, unsigned short* codes, PngHuffScratch& h) {
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < kPngSyms + 2; i += kPngDeflateThreads) h.num[i] = 0;
    int n = 0;
    for (int sym = tid; sym < nsym; sym += kPngDeflateThreads) {
        const unsigned fq = freq[sym];
        int rank = 0; n = 0;
        for (int j = 0; j < nsym; ++j) {
            const unsigned fj = freq[j];
            n += fj > 0;
            rank += (fj > 0) && (fj < fq || (fj == fq && j < sym));
        }
        h.rank[sym] = (unsigned short)rank;
        if (fq > 0) h.w[rank] = fq;
    }
    if (tid == 0) h.n = n;                          // thread 0 always owns symbol 0, so it went through the loop
    __syncthreads();
    n = h.n;
    if (tid == 0 && n >= 2) {
        int i = 0, j = n;
        for (int k = n; k < 2 * n - 1; ++k) {
            int pick[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (i < n && (j >= k || h.w[i] <= h.w[j])) pick[q] = i++;
                else pick[q] = j++;
            }
            h.w[k] = h.w[pick[0]] + h.w[pick[1]];
            h.parent[pick[0]] = (unsigned short)k; h.parent[pick[1]] = (unsigned short)k;
        }
        h.depth[2 * n - 2] = 0;
        for (int x = 2 * n - 3; x >= n; --x) h.depth[x] = (unsigned short)(h.depth[h.parent[x]] + 1);
    }
    __syncthreads();
    for (int x = tid; x < n; x += kPngDeflateThreads) atomicAdd(&h.num[n >= 2 ? h.depth[h.parent[x]] + 1 : 1], 1u);
    __syncthreads();
    if (tid == 0) {
        bool over = false;
        for (int d = limit + 1; d <= n; ++d) if (h.num[d]) { h.num[limit] += h.num[d]; over = true; }
        if (over) {
            unsigned total = 0;
            for (int l = 1; l <= limit; ++l) total += h.num[l] << (limit - l);
            while (total != (1u << limit)) {
                h.num[limit] -= 1;
                for (int l = limit - 1; l > 0; --l)
                    if (h.num[l]) { h.num[l] -= 1; h.num[l + 1] += 2; break; }
                total -= 1;
            }
        }
        unsigned c = 0, code = 0;
        h.cum[0] = 0; h.next[0] = 0;
        for (int l = 1; l <= 16; ++l) {
            code = (code + (l - 1 >= 1 && l - 1 <= limit ? h.num[l - 1] : 0u)) << 1;
            h.next[l] = code;
            if (l <= limit) c += h.num[l];
            h.cum[l] = c;
        }
    }
    __syncthreads();
    for (int sym = tid; sym < nsym; sym += kPngDeflateThreads) {
        int len = 0;
        if (freq[sym] > 0) {
            const unsigned k = (unsigned)(n - 1 - h.rank[sym]);          // 0: the most frequent symbol
            len = 1;
            while (len < limit && h.cum[len] <= k) ++len;
        }
        lens[sym] = (uint8_t)len;
    }
    __syncthreads();
    for (int sym = tid; sym < nsym; sym += kPngDeflateThreads) {
        const int len = lens[sym];
        unsigned code = 0;
        if (len) {
            code = h.next[len];
            for (int j = 0; j < sym; ++j) code += lens[j] == len;
            code = __brev(code) >> (32 - len);
        }
        codes[sym] = (unsigned short)code;
    }
    __syncthreads();
}

// value in nb <= 25 bits at bit `pos` of the LSB-first stream kept in 32-bit words
__device__ __forceinline__ void png_put_atomic(unsigned* out, int pos, unsigned value, int nb) {
    if (nb == 0) return;
    const unsigned long long x = (unsigned long long)value << (pos & 31);
    atomicOr(&out[pos >> 5], (unsigned)x);
    if (x >> 32) atomicOr(&out[(pos >> 5) + 1], (unsigned)(x >> 32));
}

// The segment in LDS.  A thread walks its own chunk of 2^shift bytes; chunks of 16 and 32 bytes start `pad` = 4 bytes further apart
// than they are long, so that the lanes of a wave, each reading its own chunk, fall on different banks (strides of 5 and 9 words).
struct PngBytes {
    uint8_t* p; int shift, pad;
    __device__ __forceinline__ int at(int i) const { return i + (i >> shift) * pad; }
    __device__ __forceinline__ int operator[](int i) const { return p[at(i)]; }
};

// The tokens of the runs that START in [lo, hi) of the segment, in order.  `next`: the first run start at or after hi (n if none).
// f(value, length, count): `count` literals (length 0) or matches of `length` at distance 1.
template <class F>
__device__ __forceinline__ void png_walk(const PngBytes data, int lo, int hi, int next, F f) {
    int i = lo;
    if (lo > 0) while (i < hi && data[i] == data[i - 1]) ++i;
    while (i < hi) {
        const int v = data[i];
        int e = i + 1;
        while (e < hi && data[e] == v) ++e;
        if (e == hi) e = next;
        const int m = e - i - 1, full = m / 258, rem = m - full * 258;
        f(v, 0, 1);
        if (full) f(v, 258, full);
        if (rem >= 3) f(v, rem, 1);
        else if (rem) f(v, 0, rem);
        i = e;
    }
}

__global__ void __launch_bounds__(kPngDeflateThreads)
png_deflate_kernel(const uint8_t* __restrict__ filtered, const PngShape s, uint8_t* __restrict__ slots, PngSegInfo* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    const int chunk = s.seg / kPngDeflateThreads;                                // bytes per thread: 1..32
    const PngBytes s_data = {s_dyn, __ffs(chunk) - 1, chunk >= 16 ? 4 : 0};       // [seg] + 4 per chunk
    unsigned* const s_out = reinterpret_cast<unsigned*>(s_dyn + s.seg + kPngDeflateThreads * 4);          // [seg + 16] bytes
    __shared__ PngHuffScratch s_h;
    __shared__ unsigned s_freq[kPngSyms + 2], s_clfreq[kPngClSyms + 1];
    __shared__ uint8_t s_len[kPngSyms + 2], s_cllen[kPngClSyms + 1];
    __shared__ unsigned short s_code[kPngSyms + 2], s_clcode[kPngClSyms + 1], s_cltok[kPngSyms + 4];
    __shared__ unsigned long long s_red[2][kPngDeflateThreads / kWave];
    __shared__ int s_fsw[kPngDeflateThreads / kWave], s_bits[kPngDeflateThreads / kWave];
    __shared__ int s_misc[8];          // 0: block has a match, 1: hlit, 2: code-length tokens, 3: hclen, 4: header bits

    const int64_t g = blockIdx.x;
    if (g >= s.T) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = (int)(g / s.S), sg = (int)(g - (int64_t)f * s.S);
    const int64_t o = (int64_t)sg * s.seg;
    const int n = (int)min((int64_t)s.seg, s.F - o);
    const bool final = sg == s.S - 1;
    const uint8_t* const src = filtered + (int64_t)f * s.Fpad + o;              // 16-byte aligned

    for (int i = tid * 16; i < n; i += kPngDeflateThreads * 16) {
        if (i + 16 <= n) {                                                       // a group never straddles two padded chunks
            const uint4 q = *reinterpret_cast<const uint4*>(src + i);
            unsigned* const w = reinterpret_cast<unsigned*>(s_dyn + s_data.at(i));
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else for (int j = i; j < n; ++j) s_dyn[s_data.at(j)] = src[j];
    }
    for (int i = tid; i < kPngSyms + 2; i += kPngDeflateThreads) s_freq[i] = 0;
    if (tid < kPngClSyms + 1) s_clfreq[tid] = 0;
    if (tid < 8) s_misc[tid] = 0;
    for (int i = tid; i < (s.seg + 16) / 4; i += kPngDeflateThreads) s_out[i] = 0;
    __syncthreads();

    // this thread's bytes, Adler partial sums, the first run start among them
    const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    unsigned long long sa = 0, sb = 0;
    int fs = n;
    for (int i = lo; i < hi; ++i) {
        const unsigned d = s_data[i];
        sa += d; sb += (unsigned long long)(n - i) * d;
        if (fs == n && (i == 0 || s_data[i - 1] != d)) fs = i;
    }
    int sfx = fs;                                                               // minimum over this and the later lanes of the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int other = __shfl_down(sfx, d);
        if (lane + d < kWave) sfx = min(sfx, other);
        sa += __shfl_xor(sa, d); sb += __shfl_xor(sb, d);
    }
    const int after = __shfl_down(sfx, 1);
    if (lane == 0) { s_fsw[wave] = sfx; s_red[0][wave] = sa; s_red[1][wave] = sb; }
    __syncthreads();
    int next = lane < kWave - 1 ? after : n;
    for (int w = wave + 1; w < kPngDeflateThreads / kWave; ++w) next = min(next, s_fsw[w]);

    png_walk(s_data, lo, hi, next, [&](int v, int length, int count) {
        int sym = v;
        if (length) { int eb, ev; png_length_code(length, sym, eb, ev); s_misc[0] = 1; }
        atomicAdd(&s_freq[sym], (unsigned)count);
    });
    if (tid == 0) s_freq[256] = 1;
    __syncthreads();

    png_huffman(s_freq, kPngSyms, 15, s_len, s_code, s_h);

    // the header's code-length sequence, run-length coded: training/png.py::code_length_tokens
    if (tid == 0) {
        int hlit = kPngSyms;
        while (s_len[hlit - 1] == 0) --hlit;                                     // >= 257: end-of-block is used
        const int total = hlit + 1, dist_len = s_misc[0] ? 1 : 0;
        int nt = 0;
        auto seq = [&](int i) { return i < hlit ? (int)s_len[i] : dist_len; };
        auto tok = [&](int sym, int extra) { s_cltok[nt++] = (unsigned short)(sym | (extra << 8)); s_clfreq[sym] += 1; };
        for (int i = 0; i < total;) {
            const int v = seq(i);
            int c = 1;
            while (i + c < total && seq(i + c) == v) ++c;
            i += c;
            if (v == 0) {
                while (c >= 11) { const int r = min(c, 138); tok(18, r - 11); c -= r; }
                if (c >= 3) { tok(17, c - 3); c = 0; }
            } else {
                tok(v, 0); --c;
                while (c >= 3) { const int r = min(c, 6); tok(16, r - 3); c -= r; }
            }
            for (; c > 0; --c) tok(v, 0);
        }
        s_misc[1] = hlit; s_misc[2] = nt;
    }
    __syncthreads();

    png_huffman(s_clfreq, kPngClSyms, 7, s_cllen, s_clcode, s_h);

    if (tid == 0) {
        int hclen = kPngClSyms;
        while (hclen > 4 && s_cllen[kPngClOrder[hclen - 1]] == 0) --hclen;
        int bits = 17 + 3 * hclen;
        for (int t = 0; t < s_misc[2]; ++t) {
            const int sym = s_cltok[t] & 255;
            bits += s_cllen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        s_misc[3] = hclen; s_misc[4] = bits;
    }

    // bits of this thread's tokens, their exclusive prefix over the workgroup (`before`) and their sum (`body`)
    int mybits = 0;
    png_walk(s_data, lo, hi, next, [&](int v, int length, int count) {
        if (length) { int sym, eb, ev; png_length_code(length, sym, eb, ev); mybits += count * (s_len[sym] + eb + 1); }
        else mybits += count * s_len[v];
    });
    int body;
    const int before = block_exclusive_scan<kPngDeflateThreads, true>(mybits, s_bits, body);          // s_bits is used here only; its barrier also publishes s_misc[3..4]
    const int header = s_misc[4];
    const int bits = header + body + s_len[256];
    const int dyn_size = final ? (bits + 7) >> 3 : ((bits + 3 + 7) >> 3) + 4;
    const bool dynamic = dyn_size < n + 5;
    const int size = dynamic ? dyn_size : n + 5;
    uint8_t* const s_outb = reinterpret_cast<uint8_t*>(s_out);

    if (dynamic) {
        if (tid == 0) {                                                         // the only writer until the barrier below
            int pos = 0;
            auto put = [&](unsigned value, int nb) { png_put_atomic(s_out, pos, value, nb); pos += nb; };
            put(final ? 1u : 0u, 1); put(2u, 2); put((unsigned)(s_misc[1] - 257), 5); put(0u, 5); put((unsigned)(s_misc[3] - 4), 4);
            for (int i = 0; i < s_misc[3]; ++i) put(s_cllen[kPngClOrder[i]], 3);
            for (int t = 0; t < s_misc[2]; ++t) {
                const int sym = s_cltok[t] & 255, extra = s_cltok[t] >> 8, l = s_cllen[sym];
                put((unsigned)s_clcode[sym] | ((unsigned)extra << l), l + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0));
            }
            png_put_atomic(s_out, header + body, s_code[256], s_len[256]);         // end-of-block
            if (!final) {                                                       // empty stored block: 000, pad, 00 00 FF FF
                const int at = (bits + 3 + 7) >> 3;
                s_outb[at + 2] = 0xff; s_outb[at + 3] = 0xff;
            }
        }
        __syncthreads();
        int pos = header + before;
        png_walk(s_data, lo, hi, next, [&](int v, int length, int count) {
            unsigned value; int nb;
            if (length) {
                int sym, eb, ev; png_length_code(length, sym, eb, ev);
                value = (unsigned)s_code[sym] | ((unsigned)ev << s_len[sym]); nb = s_len[sym] + eb + 1;          // + the distance code 0
            } else { value = s_code[v]; nb = s_len[v]; }
            for (int k = 0; k < count; ++k, pos += nb) png_put_atomic(s_out, pos, value, nb);
        });
    } else {
        if (tid == 0) {
            s_outb[0] = final ? 1 : 0;
            s_outb[1] = (uint8_t)n; s_outb[2] = (uint8_t)(n >> 8); s_outb[3] = (uint8_t)~n; s_outb[4] = (uint8_t)(~n >> 8);
        }
        for (int i = tid; i < n; i += kPngDeflateThreads) s_outb[5 + i] = s_data[i];
    }
    __syncthreads();
    uint8_t* const slot = slots + g * (int64_t)(s.seg + kPngSlotPad);           // 16-byte aligned; size <= seg + 5
    for (int i = tid * 16; i < size; i += kPngDeflateThreads * 16)
        *reinterpret_cast<uint4*>(slot + i) = *reinterpret_cast<const uint4*>(s_outb + i);
    if (tid == 0) {
        unsigned long long a = 0, b = 0;
        for (int w = 0; w < kPngDeflateThreads / kWave; ++w) { a += s_red[0][w]; b += s_red[1][w]; }
        PngSegInfo r;
        r.size = (unsigned)size; r.a = (unsigned)((1 + a) % kAdler); r.b = (unsigned)((n + b) % kAdler); r.pad = 0;
        info[g] = r;
    }
}

// ---- stage c: scan and compact ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kPngThreads)
png_compact_kernel(const uint8_t* __restrict__ slots, const PngSegInfo* __restrict__ info, const long long* __restrict__ pos,
                   const long long* __restrict__ offsets, const PngShape s, uint8_t* __restrict__ out, int64_t out_capacity) {
    __shared__ unsigned long long s_red[2][kPngThreads / kWave];
    const int64_t g = blockIdx.x;
    if (g >= s.T) return;
    const int tid = (int)threadIdx.x;
    const int f = (int)(g / s.S), sg = (int)(g - (int64_t)f * s.S);
    const int size = (int)info[g].size;
    const int64_t at = pos[g];
    if (size > s.seg + 5 || at < 2 || at + size + 4 > out_capacity) return;      // cannot happen for sizes this call's deflate wrote
    const uint8_t* const slot = slots + g * (int64_t)(s.seg + kPngSlotPad);
    copy_slot_bytes(out + at, slot, size, tid, kPngThreads);          // reads the slot below size + 16 <= seg + 21: kPngSlotPad covers it

    if (sg != 0) return;
    // the frame's Adler-32 from its segments' partial sums: with (A_k, B_k) of segment k on its own, n_k bytes at offset o_k of F,
    // A = 1 + sum (A_k - 1), B = F + sum (B_k - n_k) + (F - o_k - n_k) (A_k - 1), all mod 65521
    unsigned long long a = 0, b = 0;
    for (int k = tid; k < s.S; k += kPngThreads) {
        const PngSegInfo q = info[(int64_t)f * s.S + k];
        const int64_t ok = (int64_t)k * s.seg;
        const unsigned long long nk = (unsigned long long)min((int64_t)s.seg, s.F - ok);
        const unsigned long long a1 = (q.a + kAdler - 1) % kAdler;
        a += a1;
        b += (q.b + kAdler - nk % kAdler) % kAdler + ((unsigned long long)(s.F - ok) - nk) % kAdler * a1 % kAdler;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = a; s_red[1][tid >> 6] = b; }
    __syncthreads();
    if (tid == 0) {
        a = 0; b = 0;
        for (int w = 0; w < kPngThreads / kWave; ++w) { a += s_red[0][w]; b += s_red[1][w]; }
        const unsigned A = (unsigned)((1 + a) % kAdler), B = (unsigned)(((unsigned long long)s.F + b) % kAdler);
        const int64_t begin = offsets[f], end = offsets[f + 1];
        if (begin >= 0 && end - 4 >= begin + 2 && end <= out_capacity) {
            out[begin] = 0x78; out[begin + 1] = 0x01;
            out[end - 4] = (uint8_t)(B >> 8); out[end - 3] = (uint8_t)B; out[end - 2] = (uint8_t)(A >> 8); out[end - 1] = (uint8_t)A;
        }
    }
}

}  // namespace ide3d

extern "C" int64_t ide3d_png_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t segment_bytes) {
    ide3d::PngShape s;
    return ide3d::png_shape(n, h, w, c, segment_bytes, s) ? ide3d::png_workspace(s) : -1;
}

extern "C" int64_t ide3d_png_out_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t segment_bytes) {
    ide3d::PngShape s;
    return ide3d::png_shape(n, h, w, c, segment_bytes, s) ? ide3d::png_worst_case(s) : -1;
}

extern "C" int ide3d_png_encode(const uint8_t* frames, int32_t n, int32_t h, int32_t w, int32_t c, int32_t filter_mode, int32_t segment_bytes,
                                void* workspace, int64_t workspace_bytes, uint8_t* out, int64_t out_capacity, int64_t* offsets, void* stream) {
    using namespace ide3d;
    PngShape s;
    IDE3D_CHECK_ARG(c == 1 || c == 3, "png_encode: %d channels: grey (1) or RGB (3) frames only", c);
    IDE3D_CHECK_ARG(segment_bytes >= kPngMinSeg && segment_bytes <= kPngMaxSeg && !(segment_bytes & (segment_bytes - 1)),
                    "png_encode: segment_bytes must be a power of two in [%d, %d] (got %d)", kPngMinSeg, kPngMaxSeg, segment_bytes);
    IDE3D_CHECK_ARG(png_shape(n, h, w, c, segment_bytes, s), "png_encode: %d frames of %d x %d x %d: an empty axis, or 2 GiB or more in one call", n, h, w, c);
    IDE3D_CHECK_ARG(filter_mode >= 0 && filter_mode <= 5, "png_encode: filter_mode must be 0..4 (forced) or 5 (adaptive), got %d", filter_mode);
    if (const int rc = check_stream_buffers("png_encode", frames, workspace, workspace_bytes, png_workspace(s), out, out_capacity, png_worst_case(s), offsets))
        return rc;
    uint8_t* const ws = static_cast<uint8_t*>(workspace);
    uint8_t* const filtered = ws;
    uint8_t* const slots = ws + png_slots_offset(s);
    PngSegInfo* const info = reinterpret_cast<PngSegInfo*>(ws + png_info_offset(s));
    long long* const pos = reinterpret_cast<long long*>(ws + png_pos_offset(s));
    const hipStream_t st = (hipStream_t)stream;
    const int wide = ptr_aligned(frames, 16) && s.row % 16 == 0;
    if (c == 1) hipLaunchKernelGGL(png_filter_kernel<1>, dim3((unsigned)(s.N * s.H)), dim3(kPngThreads), 0, st, frames, s, (int)filter_mode, wide, filtered);
    else hipLaunchKernelGGL(png_filter_kernel<3>, dim3((unsigned)(s.N * s.H)), dim3(kPngThreads), 0, st, frames, s, (int)filter_mode, wide, filtered);
    IDE3D_CHECK_LAUNCH("png_filter");
    const size_t lds = (size_t)2 * s.seg + kPngDeflateThreads * 4 + 16;
    // the 32 KiB form passes 64 KiB of LDS; two workgroups still fit a CU
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(png_deflate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)s.T), dim3(kPngDeflateThreads), lds, st, filtered, s, slots, info);
    IDE3D_CHECK_LAUNCH("png_deflate");
    // 78 01 and the Adler-32 per frame, the first two in front of the frame's first segment; PngSegInfo is 4 words, `size` the first
    hipLaunchKernelGGL(segment_positions_kernel, dim3(1), dim3(kScanThreads), 0, st, reinterpret_cast<const unsigned*>(info), 4, s.T, (int64_t)s.S,
                       (int64_t)s.N, 6, 0, 2, pos, reinterpret_cast<long long*>(offsets));
    IDE3D_CHECK_LAUNCH("png_scan");
    hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)s.T), dim3(kPngThreads), 0, st, slots, info, pos, reinterpret_cast<const long long*>(offsets),
                       s, out, out_capacity);
    IDE3D_CHECK_LAUNCH("png_compact");
    return IDE3D_OK;
}
