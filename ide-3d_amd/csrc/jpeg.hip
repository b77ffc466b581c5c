// jpeg.hip — the entropy-coded scan of a baseline JPEG file from uint8 frames on the device: the compression
// behind `video_render.write_avi` (Motion-JPEG in AVI, standing in for imageio / libx264 of gen_videos.py:108,131) and `.jpg` stills.
// training/jpeg.py states the stream in integers (colour matrix, chroma average, the DCT table with its two shifts, the quantiser's
// rounding, the Huffman tables, restart intervals, padding and stuffing); every kernel here reproduces those integers, so device and host
// files are equal byte for byte.  Integer arithmetic only.
//
//   interval  one workgroup per restart interval, 32 blocks (whole MCUs: 5 / 10 / 32 for 4:2:0 / 4:4:4 RGB / grey) at a time:
//             thread (block, row): pixels -> component samples (edge replication by clamping the coordinates) -> row transform into LDS;
//             thread (block, column): column transform, quantise, zig-zag into LDS; then a wave per block, a lane per coefficient:
//             zero runs from a 64-bit ballot, code + amplitude (ZRLs in front, EOB on lane 63), a wave scan of the bit counts; the blocks'
//             totals summed over the chunk; bits ORed MSB-first into LDS words; whole bytes stuffed (FF -> FF 00, counted and scanned
//             over the workgroup) into the interval's slot of the workspace, the 0..7 bits left over carried to the next chunk.
//             Coefficients never reach HBM.  The default restart interval is one chunk, so the loop runs once.
//   scan      segment_positions_kernel (block_scan.h): the position of every interval in `out` (2 bytes per RSTm), `offsets`
//   compact   one workgroup per interval: slot -> out, RSTm after every interval but a frame's last
//
// Worst case: a block is at most 20 bits of DC (9-bit code + 11-bit amplitude) and 63 x 26 bits of AC (16-bit code + 10-bit amplitude; a
// ZRL spends 11 bits on 16 zeros, less than their 16 x 26) = 1658 bits.  An interval of b blocks is at most ceil(1658 b / 8) bytes with its
// 1-bit padding, twice that when every byte is FF and stuffed, plus 2 for RSTm: the slot size and ide3d_jpeg_out_bytes follow from it.
//
// LDS atomics (integer or) only where the result does not depend on order: two runs are bit-equal.
#include "block_scan.h"

namespace ide3d {

constexpr int kJpegThreads = 256;
constexpr int kJpegWaves = kJpegThreads / kWave;
constexpr int kJpegChunk = 32;                           // blocks per pass: 8 rows each = one thread per (block, row)
constexpr int kJpegPerWave = kJpegChunk / kJpegWaves;    // blocks a wave codes per pass
constexpr int kJpegBlockBits = 20 + 63 * 26;
constexpr int kJpegBitWords = (kJpegChunk * kJpegBlockBits + 7 + 31) / 32 + 3;          // 7 carried bits; a put touches 3 words

struct JpegShape {
    int N, H, W, C;
    int mode;            // 0 grey, 1 RGB 4:4:4, 2 RGB 4:2:0
    int mx;              // MCU columns
    int bpm;             // blocks per MCU
    int R;               // restart interval in MCUs
    int chunk;           // MCUs per pass
    int I;               // intervals per frame
    int64_t mcus;        // per frame
    int64_t T;           // N * I
    int64_t slot;        // bytes per interval slot (a multiple of 16)
    int64_t worst;       // bytes per frame, worst case
};

// T.81 Annex K: quantisation tables K.1 / K.2 (natural order), Huffman tables K.3 - K.6 as (codes per length 1..16, symbols in code order)
__constant__ uint8_t kJpegBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
__constant__ uint8_t kJpegHuffBits[4][16] = {          // DC luminance, DC chrominance, AC luminance, AC chrominance
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
__constant__ uint8_t kJpegHuffVals[4][162] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
// natural index 8 v + u -> position in the zig-zag scan
__constant__ uint8_t kJpegZigzagPos[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
                                           10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
// round(2^13 c(u) / 2 cos((2 x + 1) u pi / 16)): training/jpeg.py::DCT_TABLE
__device__ constexpr int kJpegDct[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896}, {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

static int64_t jpeg_interval_worst(int64_t blocks) { return 2 * ((kJpegBlockBits * blocks + 7) / 8) + 2; }

static bool jpeg_shape(int32_t N, int32_t H, int32_t W, int32_t C, int32_t sub, int32_t R, JpegShape& s) {
    if (N < 1 || H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return false;
    if ((sub != 444 && sub != 420) || (sub == 420 && C == 1)) return false;
    if (R < 1 || R > 65535) return false;
    s.N = N; s.H = H; s.W = W; s.C = C; s.R = R;
    s.mode = C == 1 ? 0 : sub == 444 ? 1 : 2;
    const int m = s.mode == 2 ? 16 : 8;
    s.bpm = s.mode == 0 ? 1 : s.mode == 1 ? 3 : 6;
    s.chunk = kJpegChunk / s.bpm;
    s.mx = (W + m - 1) / m;
    s.mcus = (int64_t)s.mx * ((H + m - 1) / m);
    s.I = (int)((s.mcus + R - 1) / R);
    s.T = (int64_t)N * s.I;
    const int64_t full = s.mcus / R, rest = s.mcus % R;
    s.worst = full * jpeg_interval_worst((int64_t)s.bpm * R) + (rest ? jpeg_interval_worst(s.bpm * rest) : 0);
    s.slot = (jpeg_interval_worst((int64_t)s.bpm * (s.mcus < R ? s.mcus : R)) + 15) / 16 * 16;
    // everything the kernels index stays below 2^31
    if ((int64_t)N * H * W * C >= (1ll << 31) || s.T * s.slot >= (1ll << 31) || (int64_t)N * s.worst >= (1ll << 31)) return false;
    return true;
}
static int64_t jpeg_sizes_offset(const JpegShape& s) { return s.T * s.slot; }
static int64_t jpeg_pos_offset(const JpegShape& s) { return jpeg_sizes_offset(s) + (s.T * 4 + 15) / 16 * 16; }
static int64_t jpeg_workspace(const JpegShape& s) { return jpeg_pos_offset(s) + (s.T * 8 + 15) / 16 * 16; }

// ---- samples ----------------------------------------------------------------------------------------------------------------------

// Component `comp` (0 Y, 1 Cb, 2 Cr) of pixel (y, x), coordinates clamped to the frame (edge replication), not level-shifted.
template <int MODE>
__device__ __forceinline__ int jpeg_sample(const uint8_t* __restrict__ frame, int H, int W, int comp, int y, int x) {
    y = min(y, H - 1); x = min(x, W - 1);
    if (MODE == 0) return frame[(int64_t)y * W + x];
    const uint8_t* const p = frame + ((int64_t)y * W + x) * 3;
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// Component of block j of an MCU, and how many blocks back the previous block of that component is
template <int MODE> __device__ __forceinline__ int jpeg_block_comp(int j) { return MODE == 0 ? 0 : MODE == 1 ? j : (j < 4 ? 0 : j - 3); }
template <int MODE> __device__ __forceinline__ int jpeg_block_back(int j) { return MODE == 0 ? 1 : MODE == 1 ? 3 : (j == 0 ? 3 : j < 4 ? 1 : 6); }

// n <= 59 bits of v at bit `pos` of the MSB-first stream kept in 32-bit words; touches words pos / 32 .. + 2
__device__ __forceinline__ void jpeg_put_bits(unsigned* out, int pos, unsigned long long v, int n) {
    if (n == 0) return;
    const unsigned long long x = v << (64 - n);
    const int sh = pos & 31, w = pos >> 5;
    const unsigned a = (unsigned)(x >> (32 + sh)), b = (unsigned)(x >> sh), c = (unsigned)(x << (32 - sh));
    if (a) atomicOr(&out[w], a);
    if (b) atomicOr(&out[w + 1], b);
    if (c) atomicOr(&out[w + 2], c);
}
__device__ __forceinline__ unsigned jpeg_byte(const unsigned* words, int i) { return (words[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

// ---- stage a: intervals -----------------------------------------------------------------------------------------------------------

template <int MODE>
__global__ void __launch_bounds__(kJpegThreads)
jpeg_interval_kernel(const uint8_t* __restrict__ frames, const JpegShape s, int quality, uint8_t* __restrict__ slots, unsigned* __restrict__ sizes) {
    __shared__ short s_tmp[kJpegChunk][64];             // row transforms, [y][u]
    __shared__ short s_coef[kJpegChunk][64];            // quantised, zig-zag order
    __shared__ unsigned s_bits[kJpegBitWords];
    __shared__ unsigned s_huff[4][256];                 // symbol -> code << 5 | length
    __shared__ unsigned short s_q[2][64];
    __shared__ int s_blockbits[kJpegChunk];
    __shared__ int s_prevdc[3];
    __shared__ int s_wave[kJpegWaves];

    const int64_t g = blockIdx.x;
    if (g >= s.T) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = (int)(g / s.I), it = (int)(g - (int64_t)f * s.I);
    const int64_t mcu0 = (int64_t)it * s.R;
    const int nm = (int)min((int64_t)s.R, s.mcus - mcu0);
    const uint8_t* const frame = frames + (int64_t)f * s.H * s.W * s.C;
    uint8_t* const slot = slots + g * s.slot;

    // the tables: Huffman codes from (bits, vals) as T.81 Annex C builds them, quantisers by the IJG rule
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (tid < (t < 2 ? 12 : 162)) {
            int cum = 0, code = 0, len = 0;
            for (int l = 1; l <= 16; ++l) {
                const int n = kJpegHuffBits[t][l - 1];
                if (tid < cum + n) { code += tid - cum; len = l; break; }
                cum += n; code = (code + n) << 1;
            }
            s_huff[t][kJpegHuffVals[t][tid]] = ((unsigned)code << 5) | (unsigned)len;
        }
    }
    if (tid < 128) {
        const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        s_q[tid >> 6][tid & 63] = (unsigned short)min(max(((int)kJpegBaseQ[tid >> 6][tid & 63] * scale + 50) / 100, 1), 255);
    }
    if (tid < 3) s_prevdc[tid] = 0;
    for (int i = tid; i < kJpegBitWords; i += kJpegThreads) s_bits[i] = 0;
    __syncthreads();

    int written = 0, carry = 0;                          // bytes in the slot; bits (0..7) already in s_bits: both uniform
    for (int c0 = 0; c0 < nm; c0 += s.chunk) {
        const int cm = min(s.chunk, nm - c0), nb = cm * s.bpm;
        const bool last = c0 + cm >= nm;
        {   // thread (block, row): samples and the row transform
            const int blk = tid >> 3, row = tid & 7;
            if (blk < nb) {
                const int64_t m = mcu0 + c0 + blk / s.bpm;
                const int j = blk % s.bpm, comp = jpeg_block_comp<MODE>(j);
                const int my = (int)(m / s.mx), mxi = (int)(m - (int64_t)my * s.mx);
                int v[8];
                if (MODE != 2) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = jpeg_sample<MODE>(frame, s.H, s.W, comp, my * 8 + row, mxi * 8 + i) - 128;
                } else if (j < 4) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = jpeg_sample<MODE>(frame, s.H, s.W, 0, my * 16 + (j >> 1) * 8 + row, mxi * 16 + (j & 1) * 8 + i) - 128;
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int y = my * 16 + 2 * row, x = mxi * 16 + 2 * i;
                        v[i] = ((jpeg_sample<MODE>(frame, s.H, s.W, comp, y, x) + jpeg_sample<MODE>(frame, s.H, s.W, comp, y, x + 1)
                                 + jpeg_sample<MODE>(frame, s.H, s.W, comp, y + 1, x) + jpeg_sample<MODE>(frame, s.H, s.W, comp, y + 1, x + 1) + 2) >> 2) - 128;
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int acc = 512;
#pragma unroll
                    for (int x = 0; x < 8; ++x) acc += kJpegDct[u][x] * v[x];
                    s_tmp[blk][row * 8 + u] = (short)(acc >> 10);
                }
            }
        }
        __syncthreads();
        {   // thread (block, column): the column transform, the quantiser, zig-zag
            const int blk = tid >> 3, u = tid & 7;
            if (blk < nb) {
                const int tab = jpeg_block_comp<MODE>(blk % s.bpm) > 0;
                int t[8];
#pragma unroll
                for (int y = 0; y < 8; ++y) t[y] = s_tmp[blk][y * 8 + u];
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    int acc = 4096;
#pragma unroll
                    for (int y = 0; y < 8; ++y) acc += kJpegDct[v][y] * t[y];
                    const int f8 = acc >> 13, q = s_q[tab][v * 8 + u];
                    int k = (abs(f8) + 4 * q) / (8 * q);
                    if (v + u > 0) k = min(k, 1023);
                    s_coef[blk][kJpegZigzagPos[v * 8 + u]] = (short)(f8 < 0 ? -k : k);
                }
            }
        }
        __syncthreads();

        // a wave per block, a lane per coefficient: this lane's bits (ZRLs, code, amplitude) and their place inside the block
        unsigned long long tok[kJpegPerWave];
        int tn[kJpegPerWave], tat[kJpegPerWave];
#pragma unroll
        for (int i = 0; i < kJpegPerWave; ++i) {
            const int blk = wave + kJpegWaves * i;           // uniform over the wave
            tok[i] = 0; tn[i] = 0; tat[i] = 0;
            if (blk >= nb) continue;
            const int j = blk % s.bpm, comp = jpeg_block_comp<MODE>(j), tab = comp > 0;
            const int coef = s_coef[blk][lane];
            const unsigned long long nzmask = __ballot(coef != 0) & ~1ull;
            int value = coef;
            if (lane == 0) {
                const int back = blk - jpeg_block_back<MODE>(j);
                value = coef - (back >= 0 ? (int)s_coef[back][0] : s_prevdc[comp]);
            }
            const int size = 32 - __clz(abs(value));         // 0 for 0
            const unsigned amp = (unsigned)(value < 0 ? value - 1 : value) & ((1u << size) - 1u);
            if (lane == 0) {
                const unsigned e = s_huff[tab][size];
                tok[i] = ((unsigned long long)(e >> 5) << size) | amp; tn[i] = (int)(e & 31) + size;
            } else if (coef != 0) {
                const unsigned long long lower = nzmask & ((1ull << lane) - 1ull);
                const int prev = lower ? 63 - __clzll((long long)lower) : 0;
                const int run = lane - prev - 1;
                const unsigned z = s_huff[2 + tab][0xF0], e = s_huff[2 + tab][((run & 15) << 4) | size];
                unsigned long long v = 0; int n = 0;
                for (int r = run >> 4; r > 0; --r) { v = (v << (z & 31)) | (z >> 5); n += (int)(z & 31); }
                tok[i] = (((v << (e & 31)) | (e >> 5)) << size) | amp; tn[i] = n + (int)(e & 31) + size;
            } else if (lane == 63) {
                const unsigned e = s_huff[2 + tab][0];
                tok[i] = e >> 5; tn[i] = (int)(e & 31);
            }
            const int inc = wave_inclusive_scan(tn[i]);
            tat[i] = inc - tn[i];
            if (lane == kWave - 1) s_blockbits[blk] = inc;
        }
        __syncthreads();
        int bits = carry;                                    // uniform: carried bits + the chunk's
        for (int b = 0; b < nb; ++b) bits += s_blockbits[b];
#pragma unroll
        for (int i = 0; i < kJpegPerWave; ++i) {
            const int blk = wave + kJpegWaves * i;
            if (blk >= nb) continue;
            int at = carry + tat[i];
            for (int b = 0; b < blk; ++b) at += s_blockbits[b];
            jpeg_put_bits(s_bits, at, tok[i], tn[i]);
        }
        const int padn = last ? (-bits) & 7 : 0;             // 1-bits up to the byte boundary at the interval's end
        if (tid == 0 && padn) jpeg_put_bits(s_bits, bits, (1ull << padn) - 1ull, padn);
        __syncthreads();

        // whole bytes -> the slot, FF followed by 00
        const int nbytes = (bits + padn) >> 3;
        const int per = (nbytes + kJpegThreads - 1) / kJpegThreads;
        const int lo = min(tid * per, nbytes), hi = min(lo + per, nbytes);
        int ff = 0;
        for (int i = lo; i < hi; ++i) ff += jpeg_byte(s_bits, i) == 255u;
        int total;
        const int before = block_exclusive_scan<kJpegThreads, true>(ff, s_wave, total);          // fresh: two barriers end every pass of this loop
        if ((int64_t)written + nbytes + total <= s.slot) {   // always: the slot is the worst case
            uint8_t* dst = slot + written + lo + before;
            for (int i = lo; i < hi; ++i) {
                const unsigned b = jpeg_byte(s_bits, i);
                *dst++ = (uint8_t)b;
                if (b == 255u) *dst++ = 0;
            }
        }
        written += nbytes + total;
        // the bits past the last whole byte open the next chunk's buffer; the last DC of every component is its first predictor
        const unsigned left = last ? 0u : jpeg_byte(s_bits, nbytes) << 24;
        const int used = (bits + padn + 31) / 32 + 3;
        if (tid < 3 && tid < (MODE == 0 ? 1 : 3)) s_prevdc[tid] = s_coef[MODE == 0 ? nb - 1 : nb - 3 + tid][0];
        __syncthreads();
        for (int i = tid; i < min(used, kJpegBitWords); i += kJpegThreads) s_bits[i] = i == 0 ? left : 0u;
        carry = bits & 7;
        __syncthreads();
    }
    if (tid == 0) sizes[g] = (unsigned)written;
}

// ---- stage b: scan and compact ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kJpegThreads)
jpeg_compact_kernel(const uint8_t* __restrict__ slots, const unsigned* __restrict__ sizes, const long long* __restrict__ pos, const JpegShape s,
                    uint8_t* __restrict__ out, int64_t out_capacity) {
    const int64_t g = blockIdx.x;
    if (g >= s.T) return;
    const int it = (int)(g % s.I);
    const int64_t size = sizes[g], at = pos[g];
    const bool marker = it != s.I - 1;
    if (size > s.slot || at < 0 || at + size + (marker ? 2 : 0) > out_capacity) return;      // cannot happen for sizes this call wrote
    const uint8_t* const slot = slots + g * s.slot;
    // reads the slot below size + 16 <= s.slot + 16: slots are multiples of 16 bytes, and the last one is followed inside the workspace by
    // the sizes section of at least 16 bytes (jpeg_sizes_offset)
    copy_slot_bytes(out + at, slot, (int)size, (int)threadIdx.x, kJpegThreads);
    if (marker && threadIdx.x == 0) { out[at + size] = 0xFF; out[at + size + 1] = (uint8_t)(0xD0 + (it & 7)); }
}

}  // namespace ide3d

extern "C" int64_t ide3d_jpeg_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t subsampling, int32_t restart_interval) {
    ide3d::JpegShape s;
    return ide3d::jpeg_shape(n, h, w, c, subsampling, restart_interval, s) ? ide3d::jpeg_workspace(s) : -1;
}

extern "C" int64_t ide3d_jpeg_out_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t subsampling, int32_t restart_interval) {
    ide3d::JpegShape s;
    return ide3d::jpeg_shape(n, h, w, c, subsampling, restart_interval, s) ? (int64_t)n * s.worst : -1;
}

extern "C" int ide3d_jpeg_encode(const uint8_t* frames, int32_t n, int32_t h, int32_t w, int32_t c, int32_t quality, int32_t subsampling,
                                 int32_t restart_interval, void* workspace, int64_t workspace_bytes, uint8_t* out, int64_t out_capacity,
                                 int64_t* offsets, void* stream) {
    using namespace ide3d;
    JpegShape s;
    IDE3D_CHECK_ARG(c == 1 || c == 3, "jpeg_encode: %d channels: grey (1) or RGB (3) frames only", c);
    IDE3D_CHECK_ARG(quality >= 1 && quality <= 100, "jpeg_encode: quality must be 1..100 (got %d)", quality);
    IDE3D_CHECK_ARG(subsampling == 444 || (subsampling == 420 && c == 3), "jpeg_encode: subsampling must be 444, or 420 with 3 channels (got %d with %d)",
                    subsampling, c);
    IDE3D_CHECK_ARG(restart_interval >= 1 && restart_interval <= 65535, "jpeg_encode: restart_interval must be 1..65535 MCUs (got %d)", restart_interval);
    IDE3D_CHECK_ARG(jpeg_shape(n, h, w, c, subsampling, restart_interval, s),
                    "jpeg_encode: %d frames of %d x %d x %d: an empty axis, a side above 65535, or 2 GiB or more in one call", n, h, w, c);
    if (const int rc = check_stream_buffers("jpeg_encode", frames, workspace, workspace_bytes, jpeg_workspace(s), out, out_capacity, (int64_t)n * s.worst, offsets))
        return rc;
    uint8_t* const ws = static_cast<uint8_t*>(workspace);
    unsigned* const sizes = reinterpret_cast<unsigned*>(ws + jpeg_sizes_offset(s));
    long long* const pos = reinterpret_cast<long long*>(ws + jpeg_pos_offset(s));
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)s.T), block(kJpegThreads);
    if (s.mode == 0) hipLaunchKernelGGL(jpeg_interval_kernel<0>, grid, block, 0, st, frames, s, (int)quality, ws, sizes);
    else if (s.mode == 1) hipLaunchKernelGGL(jpeg_interval_kernel<1>, grid, block, 0, st, frames, s, (int)quality, ws, sizes);
    else hipLaunchKernelGGL(jpeg_interval_kernel<2>, grid, block, 0, st, frames, s, (int)quality, ws, sizes);
    IDE3D_CHECK_LAUNCH("jpeg_interval");
    // RSTm: 2 bytes between two intervals of one frame
    hipLaunchKernelGGL(segment_positions_kernel, dim3(1), dim3(kScanThreads), 0, st, sizes, 1, s.T, (int64_t)s.I, (int64_t)s.N, 0, 2, 0, pos,
                       reinterpret_cast<long long*>(offsets));
    IDE3D_CHECK_LAUNCH("jpeg_scan");
    hipLaunchKernelGGL(jpeg_compact_kernel, grid, block, 0, st, ws, sizes, pos, s, out, out_capacity);
    IDE3D_CHECK_LAUNCH("jpeg_compact");
    return IDE3D_OK;
}
