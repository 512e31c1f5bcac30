// Baseline JPEG (SOF0, 8 bit, one interleaved sequential scan) decoder for whole batches of frames: a Motion-JPEG clip
// becomes a device tensor without a host decode loop.  The host parses the headers (mjpeg.parse_jpeg) into one
// amav_jpeg_frame record per frame; the entropy-coded data stays where it lies in the stream buffer.
//
//   markers  one wave per frame: byte-parallel search for RSTn / EOI, 512 bytes per trip; a lane's marker takes its
//            index from the ballot of the lanes before it plus the running total -> interval starts / ends in stream
//            order.
//   entropy  one lane per restart interval, 64 intervals of one frame per workgroup (= one wave).  The frame's Huffman
//            tables are expanded into 9-bit lookup tables in LDS.  The lanes decode one block each into an LDS row,
//            then the wave copies the 64 rows out 16 bytes per lane (and clears them for the next block).
//   idct     one lane per coefficient column, then per pixel row, of a block; eight blocks per wave (the encoder's
//            transform kernel run backwards) -> fp32 component planes, clamped to [0, 255].
//   colour   one thread per pixel: 4:2:0 chroma through the triangle filter, YCbCr -> RGB, round, clamp.
// No float atomics (the status words take integer atomicOr), no host synchronisation, no memset: every output element
// is written by exactly one lane.
#include <algorithm>

#include "amav_common.h"
#include "jpeg_tables.h"
#include "wave_ops.h"

// include/amav.h states the pixel arithmetic product by product; where a product is fused with an addition it is an
// explicit fmaf, nothing else contracts
#pragma clang fp contract(off)

namespace amav {
namespace jpeg_decode {

using jpeg::d_zigzag_pos;
using jpeg::kLevelStride;

struct Geom {
    int F, H, W;
    int ncomp, s420;
    int mcux, mcuy, mcus, bpm, bpf;  // MCUs per row / column / frame, blocks per MCU / frame
    int pw, ph;                      // luma plane (whole MCUs)
    int cw, ch;                      // one chroma plane as stored (whole blocks); 0 for one component
    int ccw, cch;                    // 4:2:0: the chroma plane proper, ceil(W/2) x ceil(H/2)
};

// MCUs per restart interval and intervals per frame of a record
__device__ __forceinline__ int interval_mcus(const Geom &g, int ri) { return (ri <= 0 || ri >= g.mcus) ? g.mcus : ri; }
__device__ __forceinline__ int interval_count(const Geom &g, int ri) {
    const int per = interval_mcus(g, ri);
    return (g.mcus + per - 1) / per;
}

// -------------------------------------------------------------------------------------------------------- markers
constexpr int kSearchTrips = 8;  // x 64 lanes: bytes per trip of the search loop

// grid: one wave per frame.  starts / ends: [F, mcus] (an interval holds at least one MCU); known[f]: intervals whose
// start and end are known (the first `known` ones).
__global__ __launch_bounds__(64) void jpeg_marker_kernel(Geom g, const uint8_t *__restrict__ stream, long long stream_bytes,
                                                         const amav_jpeg_frame *__restrict__ records,
                                                         long long *__restrict__ starts, long long *__restrict__ ends,
                                                         int *__restrict__ known, int *__restrict__ status) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const long long begin = clampll(records[f].scan_begin, 0, stream_bytes);
    const long long end = clampll(records[f].scan_end, begin, stream_bytes);
    const int I = interval_count(g, records[f].restart_interval);
    long long *st = starts + (size_t)f * g.mcus, *en = ends + (size_t)f * g.mcus;
    if (lane == 0) st[0] = begin;
    int total = 0;  // markers so far (wave-uniform)
    bool eoi = false, out_of_turn = false;
    for (long long base = begin; base < end && !eoi; base += 64 * kSearchTrips) {
        unsigned c0[kSearchTrips], c1[kSearchTrips];
#pragma unroll
        for (int s = 0; s < kSearchTrips; ++s) {
            const long long p = base + s * 64 + lane;
            c0[s] = p < end ? stream[p] : 0u;
            c1[s] = p + 1 < end ? stream[p + 1] : 0u;
        }
#pragma unroll
        for (int s = 0; s < kSearchTrips; ++s) {
            const long long p = base + s * 64 + lane;
            const bool is_rst = !eoi && c0[s] == 0xffu && (c1[s] & 0xf8u) == 0xd0u;
            const bool is_eoi = !eoi && c0[s] == 0xffu && c1[s] == 0xd9u;
            unsigned long long markers = __ballot(is_rst || is_eoi);
            const unsigned long long eois = __ballot(is_eoi);
            if (eois) {  // nothing after the first EOI belongs to the frame
                const int first = __ffsll((long long)eois) - 1;
                markers &= first == 63 ? ~0ull : (2ull << first) - 1ull;
                eoi = true;
            }
            if ((markers >> lane) & 1ull) {
                const int k = total + __popcll(markers & ((1ull << lane) - 1ull));
                if (k < I) en[k] = p;
                if (is_rst) {
                    if (k + 1 < I) st[k + 1] = p + 2;
                    out_of_turn |= c1[s] != (0xd0u | (unsigned)(k & 7));
                }
            }
            total += __popcll(markers);
        }
    }
    const bool any_out_of_turn = __ballot(out_of_turn) != 0;
    if (lane == 0) {
        if (!eoi && total < I) en[total] = end;  // the data stops without a marker: the last interval runs to its end
        known[f] = std::min(I, eoi ? total : total + 1);
        status[f] = (eoi && total == I && !any_out_of_turn) ? 0 : AMAV_JPEG_STATUS_MARKERS;
    }
}

// -------------------------------------------------------------------------------------------------------- entropy
constexpr int kLookBits = 9;

struct HuffmanLds {
    unsigned short look[6][1 << kLookBits];  // [component * 2 + class][next 9 bits] = length << 8 | symbol, 0: longer
    int first_code[6][17], first_val[6][17], count[6][17];  // per code length 1..16
    unsigned char dc_val[3][16], ac_val[3][256];
};

// Bits of one interval, most significant first; `acc` holds `n` valid bits in its low end.  Bytes come from
// stream[p .. end): FF 00 is the byte FF, any other FF ends the data (a marker, or fill bytes before one).
struct BitReader {
    const uint8_t *stream;
    long long p, end;
    unsigned long long acc;
    int n;

    __device__ __forceinline__ void fetch() {  // up to four more bytes
        unsigned b[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) b[t] = p + t < end ? stream[p + t] : 0x100u;  // 0x100: beyond the interval
        bool skip = false, stop = false;
        int used = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (stop) continue;
            if (skip) {  // the 00 of FF 00
                skip = false, used = t + 1;
                continue;
            }
            const unsigned v = b[t];
            if (v > 0xffu || (v == 0xffu && b[t + 1] != 0u)) {
                end = p + t, stop = true;
                continue;
            }
            skip = v == 0xffu;
            acc = acc << 8 | v, n += 8, used = t + 1;
        }
        if (skip) used = 5;
        p += used;
    }
    __device__ __forceinline__ void refill() {  // at least 33 bits unless the data ends
        while (n <= 32 && p < end) fetch();
    }
    __device__ __forceinline__ unsigned peek16() const {  // zero-padded past the end
        return (unsigned)(n >= 16 ? acc >> (n - 16) : acc << (16 - n)) & 0xffffu;
    }
    __device__ __forceinline__ bool take(int size, int &value) {  // size 0..15
        value = 0;
        if (size == 0) return true;
        if (size > n) return false;
        n -= size;
        value = (int)((acc >> n) & ((1ull << size) - 1ull));
        return true;
    }
};

__device__ __forceinline__ int extend(int bits, int size) {  // T.81 F.2.2.1
    return size == 0 || (bits >> (size - 1)) ? bits : bits - (1 << size) + 1;
}

// next Huffman symbol of table `t`, or -1: no code matches, or the data ends inside it
__device__ __forceinline__ int next_symbol(BitReader &r, const HuffmanLds &h, int t, const unsigned char *vals, int val_mask) {
    r.refill();
    const unsigned bits = r.peek16();
    const unsigned e = h.look[t][bits >> (16 - kLookBits)];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (len == 0) {
        for (int l = kLookBits + 1; l <= 16 && len == 0; ++l) {
            const int d = (int)(bits >> (16 - l)) - h.first_code[t][l];
            if (d >= 0 && d < h.count[t][l]) len = l, sym = vals[(h.first_val[t][l] + d) & val_mask];
        }
        if (len == 0) return -1;
    }
    if (len > r.n) return -1;
    r.n -= len;
    return sym;
}

__device__ __forceinline__ short saturate16(int v) { return (short)std::min(std::max(v, -32768), 32767); }

// grid: (ceil(mcus / 64), F) workgroups of one wave; lane = interval.
__global__ __launch_bounds__(64) void jpeg_entropy_decode_kernel(Geom g, const uint8_t *__restrict__ stream,
                                                                 long long stream_bytes,
                                                                 const amav_jpeg_frame *__restrict__ records,
                                                                 const long long *__restrict__ starts,
                                                                 const long long *__restrict__ ends,
                                                                 const int *__restrict__ known, short *__restrict__ levels,
                                                                 int *__restrict__ status) {
    __shared__ HuffmanLds h;
    __shared__ __attribute__((aligned(16))) short lv[64 * kLevelStride];
    __shared__ int dst_block[64];
    const int f = blockIdx.y, lane = threadIdx.x;
    const amav_jpeg_frame &rec = records[f];
    const int per = interval_mcus(g, rec.restart_interval), I = interval_count(g, rec.restart_interval);
    if ((int)blockIdx.x * 64 >= I) return;  // whole wave
    const int iv = blockIdx.x * 64 + lane;

    // tables: per code length the first code, its index into the values and the count (T.81 Annex C), then the lookup
    for (int i = lane; i < 3 * 16; i += 64) h.dc_val[i >> 4][i & 15] = rec.dc_values[i];
    for (int i = lane; i < 3 * 256; i += 64) h.ac_val[i >> 8][i & 255] = rec.ac_values[i];
    if (lane < 6) {
        const uint8_t *counts = (lane & 1 ? rec.ac_counts : rec.dc_counts) + (lane >> 1) * 16;
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
            const int c = counts[l - 1];
            h.first_code[lane][l] = code, h.first_val[lane][l] = k, h.count[lane][l] = c;
            code = (code + c) << 1, k += c;
        }
    }
    wave_sync();
    for (int i = lane; i < 6 << kLookBits; i += 64) {
        const int t = i >> kLookBits, bits = i & ((1 << kLookBits) - 1);
        unsigned short e = 0;
        for (int l = 1; l <= kLookBits && e == 0; ++l) {
            const int d = (bits >> (kLookBits - l)) - h.first_code[t][l];
            if (d >= 0 && d < h.count[t][l]) {
                const int at = h.first_val[t][l] + d;
                e = (unsigned short)(l << 8 | (t & 1 ? h.ac_val[t >> 1][at & 255] : h.dc_val[t >> 1][at & 15]));
            }
        }
        h.look[t][bits] = e;
    }
    for (int i = lane; i < 64 * kLevelStride / 2; i += 64) reinterpret_cast<unsigned *>(lv)[i] = 0u;

    const bool active = iv < I;
    const int m0 = active ? iv * per : 0;
    const int nblk = active ? std::min(per, g.mcus - m0) * g.bpm : 0;
    const bool located = active && iv < known[f];
    bool failed = !located;  // an interval the marker search did not find is zero levels (its status bit is set there)
    BitReader r{stream, 0, 0, 0ull, 0};
    if (located) {
        r.p = clampll(starts[(size_t)f * g.mcus + iv], 0, stream_bytes);
        r.end = clampll(ends[(size_t)f * g.mcus + iv], r.p, stream_bytes);
    }
    int pred0 = 0, pred1 = 0, pred2 = 0;
    short *mine = lv + lane * kLevelStride;
    const int rounds = per * g.bpm;  // blocks of a whole interval: wave-uniform
    wave_sync();
    for (int i = 0; i < rounds; ++i) {
        if (i < nblk && !failed) {
            const int k = i % g.bpm;
            const int comp = g.ncomp == 1 ? 0 : (g.s420 ? (k < 4 ? 0 : k - 3) : k);
            bool ok = true;
            int size = next_symbol(r, h, comp * 2, h.dc_val[comp], 15), bits = 0;
            ok = size >= 0 && size <= 15 && r.take(size, bits);
            if (ok) {
                const int diff = extend(bits, size);
                const int dc = (comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2)) + diff;
                if (comp == 0) pred0 = dc; else if (comp == 1) pred1 = dc; else pred2 = dc;
                mine[0] = saturate16(dc);
                int pos = 1;
                while (pos < 64) {
                    const int rs = next_symbol(r, h, comp * 2 + 1, h.ac_val[comp], 255);
                    if (rs < 0) {
                        ok = false;
                        break;
                    }
                    const int run = rs >> 4;
                    size = rs & 15;
                    if (size == 0) {
                        if (run == 15) {  // ZRL
                            pos += 16;
                            continue;
                        }
                        ok = run == 0;  // EOB; EOBn belongs to progressive scans
                        break;
                    }
                    pos += run;
                    if (pos > 63 || !r.take(size, bits)) {
                        ok = false;
                        break;
                    }
                    mine[pos++] = (short)extend(bits, size);
                }
            }
            if (!ok) {
                failed = true;
                for (int w = 0; w < kLevelStride / 2; ++w) reinterpret_cast<unsigned *>(mine)[w] = 0u;
            }
        }
        dst_block[lane] = i < nblk ? 1 : 0;
        wave_sync();
        // the 64 rows leave 16 bytes per lane: 8 lanes per block, 128 contiguous bytes each
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int c = t * 64 + lane, owner = c >> 3, part = c & 7;
            unsigned *src = reinterpret_cast<unsigned *>(lv + owner * kLevelStride + part * 8);
            const uint4 v = make_uint4(src[0], src[1], src[2], src[3]);
            src[0] = 0u, src[1] = 0u, src[2] = 0u, src[3] = 0u;
            // the owner's block0 + i: its interval is blockIdx.x * 64 + owner
            const long long ob = (long long)f * g.bpf + ((long long)(blockIdx.x * 64 + owner) * per) * g.bpm + i;
            if (dst_block[owner]) *reinterpret_cast<uint4 *>(levels + (size_t)ob * 64 + part * 8) = v;
        }
        wave_sync();
    }
    if (located && failed) atomicOr(&status[f], AMAV_JPEG_STATUS_ENTROPY);
}

// ----------------------------------------------------------------------------------------------------------- idct
// orthonormal 8-point inverse DCT (DCT-III), even / odd halves: c(j) = cos(j pi / 16) / 2
__device__ __forceinline__ void idct8(const float (&X)[8], float (&x)[8]) {
    constexpr float c1 = 0.49039264020161522f, c2 = 0.46193976625564337f, c3 = 0.41573480615127262f,
                    c4 = 0.35355339059327379f, c5 = 0.27778511650980114f, c6 = 0.19134171618254489f,
                    c7 = 0.09754516100806417f;
    const float e0 = fmaf(c6, X[6], fmaf(c4, X[4], fmaf(c2, X[2], c4 * X[0])));
    const float e1 = fmaf(-c2, X[6], fmaf(-c4, X[4], fmaf(c6, X[2], c4 * X[0])));
    const float e2 = fmaf(c2, X[6], fmaf(-c4, X[4], fmaf(-c6, X[2], c4 * X[0])));
    const float e3 = fmaf(-c6, X[6], fmaf(c4, X[4], fmaf(-c2, X[2], c4 * X[0])));
    const float o0 = fmaf(c7, X[7], fmaf(c5, X[5], fmaf(c3, X[3], c1 * X[1])));
    const float o1 = fmaf(-c5, X[7], fmaf(-c1, X[5], fmaf(-c7, X[3], c3 * X[1])));
    const float o2 = fmaf(c3, X[7], fmaf(c7, X[5], fmaf(-c1, X[3], c5 * X[1])));
    const float o3 = fmaf(-c1, X[7], fmaf(c3, X[5], fmaf(-c5, X[3], c7 * X[1])));
    x[0] = e0 + o0, x[7] = e0 - o0;
    x[1] = e1 + o1, x[6] = e1 - o1;
    x[2] = e2 + o2, x[5] = e2 - o2;
    x[3] = e3 + o3, x[4] = e3 - o3;
}

// grid: 4 waves per workgroup, 8 blocks per wave; lane = 8 * (block in wave) + (coefficient column, later pixel row)
__global__ __launch_bounds__(256) void jpeg_idct_kernel(Geom g, const short *__restrict__ levels,
                                                        const amav_jpeg_frame *__restrict__ records,
                                                        float *__restrict__ luma, float *__restrict__ chroma, long long total) {
    __shared__ float tr[4][8][8][9];
    __shared__ __attribute__((aligned(16))) short staged[4][8 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane >> 3, r = lane & 7;
    const long long first = ((long long)blockIdx.x * 4 + wave) * 8;
    if (first >= total) return;  // whole wave (no workgroup barrier below)
    const bool live = first + j < total;
    // the wave's 8 blocks are 1 KiB of contiguous levels: 16 bytes per lane
    uint4 in = make_uint4(0u, 0u, 0u, 0u);
    if (live) in = *reinterpret_cast<const uint4 *>(levels + (size_t)first * 64 + lane * 8);
    *reinterpret_cast<uint4 *>(staged[wave] + lane * 8) = in;
    const long long b = std::min(first + j, total - 1);
    const int f = (int)(b / g.bpf);
    const int i = (int)(b - (long long)f * g.bpf), m = i / g.bpm, k = i - m * g.bpm;
    const int my = m / g.mcux, mx = m - my * g.mcux;
    const int comp = g.ncomp == 1 ? 0 : (g.s420 ? (k < 4 ? 0 : k - 3) : k);
    const uint8_t *q = records[f].quant + comp * 64;
    wave_sync();
    float X[8], t[8], px[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) {  // coefficient (vertical frequency v, horizontal frequency r)
        const int zz = d_zigzag_pos.at[v * 8 + r];
        X[v] = (float)staged[wave][j * 64 + zz] * (float)q[zz];
    }
    idct8(X, t);  // t[y] at horizontal frequency r
#pragma unroll
    for (int y = 0; y < 8; ++y) tr[wave][j][y][r] = t[y];
    wave_sync();
#pragma unroll
    for (int u = 0; u < 8; ++u) X[u] = tr[wave][j][r][u];  // the lane now owns pixel row r
    idct8(X, px);
#pragma unroll
    for (int x = 0; x < 8; ++x) px[x] = fminf(fmaxf(px[x] + 128.0f, 0.0f), 255.0f);
    if (!live) return;
    float *dst;
    if (comp == 0) {
        const int by = g.s420 ? my * 2 + (k >> 1) : my, bx = g.s420 ? mx * 2 + (k & 1) : mx;
        dst = luma + ((size_t)f * g.ph + by * 8 + r) * g.pw + bx * 8;
    } else {
        dst = chroma + (((size_t)f * 2 + (comp - 1)) * g.ch + my * 8 + r) * g.cw + mx * 8;
    }
    reinterpret_cast<float4 *>(dst)[0] = make_float4(px[0], px[1], px[2], px[3]);
    reinterpret_cast<float4 *>(dst)[1] = make_float4(px[4], px[5], px[6], px[7]);
}

// --------------------------------------------------------------------------------------------------------- colour
__device__ __forceinline__ float to8(float v) { return fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

// 4:2:0 chroma at pixel (y, x): 3/4 of the nearer sample, 1/4 of the farther, vertically then horizontally
__device__ __forceinline__ float triangle(const float *__restrict__ plane, const Geom &g, int y, int x) {
    const int cy = y >> 1, cx = x >> 1;
    const int ny = std::min(std::max(cy + ((y & 1) ? 1 : -1), 0), g.cch - 1);
    const int nx = std::min(std::max(cx + ((x & 1) ? 1 : -1), 0), g.ccw - 1);
    const float near_col = fmaf(0.25f, plane[(size_t)ny * g.cw + cx], 0.75f * plane[(size_t)cy * g.cw + cx]);
    const float far_col = fmaf(0.25f, plane[(size_t)ny * g.cw + nx], 0.75f * plane[(size_t)cy * g.cw + nx]);
    return fmaf(0.25f, far_col, 0.75f * near_col);
}

template <bool kChwF32>
__global__ __launch_bounds__(256) void jpeg_colour_kernel(Geom g, const float *__restrict__ luma,
                                                          const float *__restrict__ chroma, void *__restrict__ out,
                                                          long long pixels) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= pixels) return;
    const long long hw = (long long)g.H * g.W;
    const int f = (int)(id / hw);
    const long long rem = id - f * hw;
    const int y = (int)(rem / g.W), x = (int)(rem - (long long)y * g.W);
    const float Y = luma[((size_t)f * g.ph + y) * g.pw + x];
    float R = Y, G = Y, B = Y;
    if (g.ncomp == 3) {
        const float *pcb = chroma + (size_t)f * 2 * g.ch * g.cw, *pcr = pcb + (size_t)g.ch * g.cw;
        float cb, cr;
        if (g.s420) {
            cb = triangle(pcb, g, y, x), cr = triangle(pcr, g, y, x);
        } else {
            cb = pcb[(size_t)y * g.cw + x], cr = pcr[(size_t)y * g.cw + x];
        }
        cb -= 128.0f, cr -= 128.0f;
        R = fmaf(1.402f, cr, Y);
        G = fmaf(-0.714136f, cr, fmaf(-0.344136f, cb, Y));
        B = fmaf(1.772f, cb, Y);
    }
    R = to8(R), G = to8(G), B = to8(B);
    if (kChwF32) {
        float *o = static_cast<float *>(out) + (size_t)f * 3 * hw + rem;
        o[0] = R / 255.0f, o[hw] = G / 255.0f, o[2 * hw] = B / 255.0f;
    } else {
        uint8_t *o = static_cast<uint8_t *>(out) + (size_t)id * 3;
        o[0] = (uint8_t)R, o[1] = (uint8_t)G, o[2] = (uint8_t)B;
    }
}

// ----------------------------------------------------------------------------------------------------------- host
static bool make_geom(int F, int H, int W, int sampling, Geom &g) {
    if (F < 1 || F > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535) return false;
    if (sampling != AMAV_JPEG_420 && sampling != AMAV_JPEG_444 && sampling != AMAV_JPEG_GRAY) return false;
    g.F = F, g.H = H, g.W = W;
    g.ncomp = sampling == AMAV_JPEG_GRAY ? 1 : 3;
    g.s420 = sampling == AMAV_JPEG_420;
    const int mcu = g.s420 ? 16 : 8;
    g.mcux = (W + mcu - 1) / mcu, g.mcuy = (H + mcu - 1) / mcu;
    g.mcus = g.mcux * g.mcuy;  // <= 8192^2
    g.bpm = g.ncomp == 1 ? 1 : (g.s420 ? 6 : 3);
    g.bpf = g.mcus * g.bpm;
    if ((long long)F * g.bpf > 0x7fffffffLL) return false;  // block indices stay in int32
    g.pw = g.mcux * mcu, g.ph = g.mcuy * mcu;
    g.cw = g.ncomp == 1 ? 0 : g.mcux * 8, g.ch = g.ncomp == 1 ? 0 : g.mcuy * 8;
    g.ccw = (W + 1) / 2, g.cch = (H + 1) / 2;
    return true;
}

struct Workspace {
    long long *starts, *ends;
    int *known;
    short *levels;
    float *luma, *chroma;
    size_t bytes;
};
static Workspace carve(const Geom &g, bool levels_only, void *base) {
    Carver c(base);
    Workspace w{};
    w.starts = c.take<long long>((size_t)g.F * g.mcus);
    w.ends = c.take<long long>((size_t)g.F * g.mcus);
    w.known = c.take<int>((size_t)g.F);
    if (!levels_only) {
        w.levels = c.take<short>((size_t)g.F * g.bpf * 64);
        w.luma = c.take<float>((size_t)g.F * g.ph * g.pw);
        w.chroma = c.take<float>((size_t)g.F * 2 * g.ch * g.cw);
    }
    w.bytes = c.total();
    return w;
}

static int check_common(const char *who, int F, int H, int W, int sampling, const uint8_t *stream, int64_t stream_bytes,
                        const void *records, const int32_t *status, Geom &g) {
    AMAV_REQUIRE(sampling == AMAV_JPEG_420 || sampling == AMAV_JPEG_444 || sampling == AMAV_JPEG_GRAY,
                 "%s: unknown sampling %d (420, 444 or 400)", who, sampling);
    AMAV_REQUIRE(F >= 1 && F <= 65535 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535,
                 "%s: sizes outside 1..65535 (F=%d H=%d W=%d)", who, F, H, W);
    AMAV_REQUIRE(make_geom(F, H, W, sampling, g), "%s: %d frames of %dx%d exceed the decoder's limits", who, F, W, H);
    return check_stream_args(who, stream, stream_bytes, records, status);
}

static void launch_levels(const Geom &g, const uint8_t *bytes, int64_t stream_bytes, const void *records, const Workspace &ws,
                          short *levels, int32_t *status, hipStream_t stream) {
    const amav_jpeg_frame *rec = static_cast<const amav_jpeg_frame *>(records);
    jpeg_marker_kernel<<<g.F, 64, 0, stream>>>(g, bytes, (long long)stream_bytes, rec, ws.starts, ws.ends, ws.known, status);
    jpeg_entropy_decode_kernel<<<dim3((g.mcus + 63) / 64, g.F), 64, 0, stream>>>(g, bytes, (long long)stream_bytes, rec,
                                                                               ws.starts, ws.ends, ws.known, levels, status);
}

}  // namespace jpeg_decode
}  // namespace amav

using namespace amav;
using namespace amav::jpeg_decode;

static_assert(sizeof(amav_jpeg_frame) == 1128, "amav_jpeg_frame is packed by the host as 1128 bytes");

extern "C" size_t amav_jpeg_decode_workspace_bytes(int F, int H, int W, int sampling, int levels_only) {
    Geom g;
    if (!make_geom(F, H, W, sampling, g)) return 0;
    return carve(g, levels_only != 0, nullptr).bytes;
}

extern "C" int amav_jpeg_decode_levels(int F, int H, int W, int sampling, const uint8_t *bytes, int64_t stream_bytes,
                                       const void *records, void *levels, size_t levels_bytes, int32_t *status,
                                       void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "amav_jpeg_decode_levels";
    Geom g;
    if (int rc = check_common(who, F, H, W, sampling, bytes, stream_bytes, records, status, g)) return rc;
    AMAV_REQUIRE(levels, "%s: NULL levels", who);
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(levels) & 15) == 0, "%s: misaligned levels", who);
    const size_t need = (size_t)F * g.bpf * 64 * sizeof(short);
    if (levels_bytes < need) return fail(AMAV_ERR_WORKSPACE, "%s: levels buffer %zu < %zu", who, levels_bytes, need);
    const Workspace ws = carve(g, true, workspace);
    if (int rc = check_workspace(who, ws.bytes, workspace, workspace_bytes)) return rc;
    launch_levels(g, bytes, stream_bytes, records, ws, static_cast<short *>(levels), status, static_cast<hipStream_t>(stream_));
    return check_launch(who);
}

extern "C" int amav_jpeg_decode(int F, int H, int W, int sampling, const uint8_t *bytes, int64_t stream_bytes,
                                const void *records, int layout, void *out, size_t out_bytes, int32_t *status,
                                void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "amav_jpeg_decode";
    Geom g;
    if (int rc = check_common(who, F, H, W, sampling, bytes, stream_bytes, records, status, g)) return rc;
    AMAV_REQUIRE(layout == AMAV_JPEG_HWC_U8 || layout == AMAV_JPEG_CHW_F32, "%s: unknown layout %d", who, layout);
    AMAV_REQUIRE(out, "%s: NULL out", who);
    AMAV_REQUIRE(layout == AMAV_JPEG_HWC_U8 || (reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: misaligned out", who);
    const size_t need = (size_t)F * H * W * 3 * (layout == AMAV_JPEG_CHW_F32 ? sizeof(float) : 1);
    if (out_bytes < need) return fail(AMAV_ERR_WORKSPACE, "%s: output buffer %zu < %zu", who, out_bytes, need);
    const Workspace ws = carve(g, false, workspace);
    if (int rc = check_workspace(who, ws.bytes, workspace, workspace_bytes)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    launch_levels(g, bytes, stream_bytes, records, ws, ws.levels, status, stream);
    const long long total = (long long)F * g.bpf, pixels = (long long)F * H * W;
    const amav_jpeg_frame *rec = static_cast<const amav_jpeg_frame *>(records);
    jpeg_idct_kernel<<<(unsigned)((total + 31) / 32), 256, 0, stream>>>(g, ws.levels, rec, ws.luma, ws.chroma, total);
    const unsigned grid = (unsigned)((pixels + 255) / 256);
    if (layout == AMAV_JPEG_CHW_F32)
        jpeg_colour_kernel<true><<<grid, 256, 0, stream>>>(g, ws.luma, ws.chroma, out, pixels);
    else
        jpeg_colour_kernel<false><<<grid, 256, 0, stream>>>(g, ws.luma, ws.chroma, out, pixels);
    return check_launch(who);
}
