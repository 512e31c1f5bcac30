// Baseline JPEG (SOF0, 8 bit, YCbCr, JFIF) encoder for whole batches of rendered frames: the demo's clip leaves the GPU
// as Motion-JPEG instead of raw rgb24.  Every frame becomes a complete JPEG file (its own DQT / DHT segments); the
// frames are packed back to back into one stream with int64 frame offsets on the device.
//
//   transform  frames -> int16 levels [F, blocks in MCU-interleaved scan order, 64 zigzag]
//              one lane per 8-pixel row of a block, eight blocks per wave: colour conversion (JFIF, fp32; 4:2:0 chroma
//              is the mean of each 2x2) -> level shift -> row DCT in registers -> transpose through LDS -> column DCT
//              -> divide by the table entry, round to nearest -> zigzag.  An MCU the caller's tile hint marks as pure
//              background takes the levels of a constant block, which the same code computed once (const_levels).
//   entropy    one wave per restart interval, in rounds of 64 blocks (one per lane): DC difference + run/size symbols
//              -> bit length per block -> wave prefix sum -> codes OR-ed into an LDS bit buffer -> bytes, with FF -> FF 00
//              stuffing.  Run twice: first only to size every interval, then (after the scan) to write the bytes at
//              their final place, so no worst-case staging buffer is needed and a short output buffer only loses bytes.
//   scan       interval sizes -> interval and frame offsets (int64), overflow flag.
// No float atomics (the bit buffer takes integer LDS atomicOr: order-independent), no host synchronisation.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "amav_common.h"
#include "jpeg_tables.h"
#include "wave_ops.h"

namespace amav {
namespace jpeg {

struct Geom {
    int F, H, W;
    int s444;      // 1: 4:4:4 (MCU 8x8, 3 blocks), 0: 4:2:0 (MCU 16x16, 6 blocks)
    int mcux, mcuy, bpm, bpf;  // MCUs per row / column, blocks per MCU / frame
    int gx, T;     // the tile hint's grid: 16x16 tiles per row, per frame
    int rr, I;     // MCU rows per restart interval, intervals per frame
};

struct QuantTables {
    uint8_t q[2][64];  // natural order
};

struct HeaderBytes {
    uint8_t b[kHeaderMax];
};

__device__ const CodeTable d_dc_codes[2] = {make_code_table(kDcBits[0], kDcVals), make_code_table(kDcBits[1], kDcVals)};
__device__ const CodeTable d_ac_codes[2] = {make_code_table(kAcBits[0], kAcVals[0]),
                                            make_code_table(kAcBits[1], kAcVals[1])};

// ------------------------------------------------------------------------------------------------------ transform
__device__ __forceinline__ float quant8f(float v) { return (float)quant8(v); }

// pixel (clamped to the image: a partial MCU replicates the last column / row) as 8-bit values in floats
__device__ __forceinline__ void load_rgb(const float4 *__restrict__ px, size_t at, float &r, float &g, float &b) {
    const float4 p = px[at];
    r = quant8f(p.x), g = quant8f(p.y), b = quant8f(p.z);  // as amav_frames_to_rgb8: clamp, x 255, truncate
}
__device__ __forceinline__ void load_rgb(const uint8_t *__restrict__ px, size_t at, float &r, float &g, float &b) {
    r = (float)px[at * 3], g = (float)px[at * 3 + 1], b = (float)px[at * 3 + 2];
}

// level-shifted sample of component `comp` (0 Y, 1 Cb, 2 Cr); every product is an explicit fmaf so that each
// instantiation rounds alike (the hinted stream must equal the unhinted one bit for bit)
__device__ __forceinline__ float ycc_sample(int comp, float r, float g, float b) {
    const float y = fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r)) - 128.0f;
    const float cb = fmaf(0.5f, b, fmaf(-0.331264f, g, -0.168736f * r));
    const float cr = fmaf(-0.081312f, b, fmaf(-0.418688f, g, 0.5f * r));
    return comp == 0 ? y : (comp == 1 ? cb : cr);
}

// orthonormal 8-point DCT-II, even / odd halves: c(j) = cos(j pi / 16) / 2
__device__ __forceinline__ void dct8(const float (&x)[8], float (&o)[8]) {
    constexpr float c1 = 0.49039264020161522f, c2 = 0.46193976625564337f, c3 = 0.41573480615127262f,
                    c4 = 0.35355339059327379f, c5 = 0.27778511650980114f, c6 = 0.19134171618254489f,
                    c7 = 0.09754516100806417f;
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    o[0] = fmaf(c4, s3, fmaf(c4, s2, fmaf(c4, s1, c4 * s0)));
    o[2] = fmaf(-c2, s3, fmaf(-c6, s2, fmaf(c6, s1, c2 * s0)));
    o[4] = fmaf(c4, s3, fmaf(-c4, s2, fmaf(-c4, s1, c4 * s0)));
    o[6] = fmaf(-c6, s3, fmaf(c2, s2, fmaf(-c2, s1, c6 * s0)));
    o[1] = fmaf(c7, d3, fmaf(c5, d2, fmaf(c3, d1, c1 * d0)));
    o[3] = fmaf(-c5, d3, fmaf(-c1, d2, fmaf(-c7, d1, c3 * d0)));
    o[5] = fmaf(c3, d3, fmaf(c7, d2, fmaf(-c1, d1, c5 * d0)));
    o[7] = fmaf(-c1, d3, fmaf(c3, d2, fmaf(-c5, d1, c7 * d0)));
}

// grid: 4 waves per workgroup, 8 blocks per wave; lane = 8 * (block in wave) + (pixel row, later coefficient column).
// kConst: the three constant blocks (Y, Cb, Cr) of the background colour, into the table hinted MCUs copy from.
template <typename Px, bool kConst>
__global__ __launch_bounds__(256) void jpeg_transform_kernel(Geom g, const Px *__restrict__ frames, QuantTables qt,
                                                             const int *__restrict__ hint, float bg_r, float bg_g,
                                                             float bg_b, const short *__restrict__ const_levels,
                                                             short *__restrict__ levels, long long total) {
    __shared__ float tr[4][8][8][9];
    __shared__ __attribute__((aligned(16))) short staged[4][8 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane >> 3, r = lane & 7;
    const long long first = ((long long)blockIdx.x * 4 + wave) * 8;
    if (first >= total) return;  // whole wave (no workgroup barrier below)
    const long long b = std::min(first + j, total - 1);
    int comp, f = 0, k = 0, mx = 0, my = 0;
    bool hinted = false;
    if (kConst) {
        comp = (int)b;
    } else {
        f = (int)(b / g.bpf);
        const int i = (int)(b - (long long)f * g.bpf), m = i / g.bpm;
        k = i - m * g.bpm;
        my = m / g.mcux, mx = m - my * g.mcux;
        comp = g.s444 ? k : (k < 4 ? 0 : k - 3);
        if (hint) {
            const int tile = g.s444 ? (my >> 1) * g.gx + (mx >> 1) : my * g.gx + mx;
            hinted = hint[(size_t)f * g.T + tile] == 0;
        }
    }
    short *out = staged[wave];
    if (__ballot(!hinted) != 0) {  // a wave of background blocks skips the arithmetic
        float s[8];
        if (kConst || hinted) {
#pragma unroll
            for (int t = 0; t < 8; ++t) s[t] = ycc_sample(comp, bg_r, bg_g, bg_b);
        } else if (g.s444 || comp == 0) {
            const int y = std::min((g.s444 ? my * 8 : my * 16 + (k >> 1) * 8) + r, g.H - 1);
            const int x0 = g.s444 ? mx * 8 : mx * 16 + (k & 1) * 8;
            const size_t row = ((size_t)f * g.H + y) * g.W;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                float pr, pg, pb;
                load_rgb(frames, row + std::min(x0 + t, g.W - 1), pr, pg, pb);
                s[t] = ycc_sample(comp, pr, pg, pb);
            }
        } else {
            const int y0 = std::min(my * 16 + 2 * r, g.H - 1), y1 = std::min(my * 16 + 2 * r + 1, g.H - 1);
            const size_t row0 = ((size_t)f * g.H + y0) * g.W, row1 = ((size_t)f * g.H + y1) * g.W;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int xa = std::min(mx * 16 + 2 * t, g.W - 1), xb = std::min(mx * 16 + 2 * t + 1, g.W - 1);
                float r0, g0, b0, r1, g1, b1, r2, g2, b2, r3, g3, b3;
                load_rgb(frames, row0 + xa, r0, g0, b0);
                load_rgb(frames, row0 + xb, r1, g1, b1);
                load_rgb(frames, row1 + xa, r2, g2, b2);
                load_rgb(frames, row1 + xb, r3, g3, b3);
                // sums of four 8-bit values are exact in fp32, so this is the mean of the 2x2 whichever way it is taken
                s[t] = ycc_sample(comp, 0.25f * ((r0 + r1) + (r2 + r3)), 0.25f * ((g0 + g1) + (g2 + g3)),
                                  0.25f * ((b0 + b1) + (b2 + b3)));
            }
        }
        float a[8], c[8], d[8];
        dct8(s, a);  // a[u] of pixel row r
#pragma unroll
        for (int u = 0; u < 8; ++u) tr[wave][j][r][u] = a[u];
        wave_sync();
#pragma unroll
        for (int y = 0; y < 8; ++y) c[y] = tr[wave][j][y][r];  // the lane now owns coefficient column u = r
        dct8(c, d);                                             // d[v]: coefficient (v, u = r)
        if (!hinted) {
            const int table = comp == 0 ? 0 : 1;
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int nat = v * 8 + r;
                const float level = rintf(d[v] / (float)qt.q[table][nat]);
                // 8-bit samples cannot exceed these; the clamp only keeps the entropy coder inside its code tables
                out[j * 64 + d_zigzag_pos.at[nat]] = (short)fminf(fmaxf(level, nat == 0 ? -1024.f : -1023.f), 1023.f);
            }
        }
    }
    if (hinted) {
#pragma unroll
        for (int t = 0; t < 8; ++t) out[j * 64 + r * 8 + t] = const_levels[comp * 64 + r * 8 + t];
    }
    wave_sync();
    if (first + j < total)  // 16 bytes per lane: the wave's 8 blocks are 1 KiB of contiguous output
        *reinterpret_cast<uint4 *>(levels + (size_t)first * 64 + lane * 8) = *reinterpret_cast<const uint4 *>(out + lane * 8);
}

// -------------------------------------------------------------------------------------------------------- entropy
constexpr int kRound = 64;                                          // blocks per round: one per lane
constexpr int kBitWords = (kRound * kMaxBlockBits + 31) / 32 + 8;   // + the carried byte and the spill word

struct BitCursor {
    unsigned *bits;
    int pos;
    // `len` (1..27) bits of `code` at bit `pos` of the big-endian bit stream (word w holds bytes 4w .. 4w + 3, first
    // byte on top); lanes own disjoint bit ranges, so OR gives the same words in any order
    __device__ __forceinline__ void put(unsigned code, int len) {
        const unsigned long long x = (unsigned long long)code << (64 - len - (pos & 31));
        const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
        atomicOr(&bits[pos >> 5], hi);
        if (lo) atomicOr(&bits[(pos >> 5) + 1], lo);
        pos += len;
    }
};

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }  // 0 for v == 0
__device__ __forceinline__ unsigned extra_bits(int v, int size) { return (unsigned)(v + (v >> 31)) & ((1u << size) - 1u); }

// Symbols of one block: kEmit = 0 returns the bit length, kEmit = 1 writes the codes through `cur`.
template <bool kEmit>
__device__ __forceinline__ int code_block(const short *__restrict__ lv, int dc_diff, const unsigned *__restrict__ dc_tab,
                                          const unsigned *__restrict__ ac_tab, BitCursor &cur) {
    int nbits = 0;
    {
        const int size = category(dc_diff);
        const unsigned e = dc_tab[size];
        if (kEmit) cur.put((e & 0xffffu) << size | extra_bits(dc_diff, size), (int)(e >> 16) + size);
        nbits += (int)(e >> 16) + size;
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = lv[k];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run >= 16) {  // ZRL
            const unsigned z = ac_tab[0xf0];
            if (kEmit) cur.put(z & 0xffffu, (int)(z >> 16));
            nbits += (int)(z >> 16);
            run -= 16;
        }
        const int size = category(v);
        const unsigned e = ac_tab[run << 4 | size];
        if (kEmit) cur.put((e & 0xffffu) << size | extra_bits(v, size), (int)(e >> 16) + size);
        nbits += (int)(e >> 16) + size;
        run = 0;
    }
    if (run > 0) {  // EOB
        const unsigned e = ac_tab[0];
        if (kEmit) cur.put(e & 0xffffu, (int)(e >> 16));
        nbits += (int)(e >> 16);
    }
    return nbits;
}

// One wave (= one workgroup) per restart interval.  kWrite = 0: sizes[interval] = bytes of its entropy-coded segment
// (stuffing included); kWrite = 1: the frame header (first interval) or the RSTn marker, the segment, and EOI after the
// frame's last interval, at offsets[interval] of the stream; nothing is stored at or beyond `cap`.
template <bool kWrite>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(Geom g, const short *__restrict__ levels,
                                                          long long *__restrict__ sizes,
                                                          const long long *__restrict__ offsets, HeaderBytes header,
                                                          int header_bytes, uint8_t *__restrict__ stream,
                                                          long long cap) {
    __shared__ unsigned bits[kBitWords];
    __shared__ __attribute__((aligned(16))) short lv[kRound * kLevelStride];
    __shared__ unsigned dc_tab[2][16], ac_tab[2][256];
    const int lane = threadIdx.x;
    const int f = blockIdx.x / g.I, iv = blockIdx.x - f * g.I;
    for (int i = lane; i < kBitWords; i += 64) bits[i] = 0;
    for (int i = lane; i < 512; i += 64) ac_tab[i >> 8][i & 255] = d_ac_codes[i >> 8].entry[i & 255];
    if (lane < 32) dc_tab[lane >> 4][lane & 15] = d_dc_codes[lane >> 4].entry[lane & 15];
    const int row0 = iv * g.rr, rows = std::min(g.rr, g.mcuy - row0);
    const int nblk = rows * g.mcux * g.bpm;
    const size_t base = (size_t)f * g.bpf + (size_t)row0 * g.mcux * g.bpm;  // first block of the interval
    long long at = 0;  // next byte of the stream
    if (kWrite) {
        at = offsets[blockIdx.x];
        if (iv == 0) {
            for (int i = lane; i < header_bytes; i += 64)
                if (at + i < cap) stream[at + i] = header.b[i];
            at += header_bytes;
        } else {
            if (lane < 2 && at + lane < cap) stream[at + lane] = lane == 0 ? 0xff : 0xd0 + ((iv - 1) & 7);
            at += 2;
        }
    }
    int carry_bits = 0;
    long long stuffed = 0;  // per lane without kWrite, wave-uniform running total with it
    long long plain = 0;    // bytes before stuffing
    wave_sync();
    for (int r0 = 0; r0 < nblk; r0 += kRound) {
        const int cnt = std::min(kRound, nblk - r0);
        // this round's levels, coalesced: 16 bytes per lane and trip -> [block][66] shorts
        const uint4 *src = reinterpret_cast<const uint4 *>(levels + (base + r0) * 64);
        for (int c = lane; c < cnt * 8; c += 64) {
            const uint4 v = src[c];
            unsigned *dst = reinterpret_cast<unsigned *>(lv + (c >> 3) * kLevelStride + (c & 7) * 8);
            dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
        }
        wave_sync();
        const int i = r0 + lane;
        const bool active = lane < cnt;
        const short *mine = lv + lane * kLevelStride;
        int nbits = 0, dc_diff = 0, table = 0;
        BitCursor cur{bits, 0};
        if (active) {
            const int k = g.s444 ? 0 : i % 6;
            const int prev = g.s444 ? i - 3 : (k == 0 ? i - 3 : (k < 4 ? i - 1 : i - 6));  // same component, this interval
            const int pred = prev >= 0 ? levels[(base + prev) * 64] : 0;
            dc_diff = mine[0] - pred;
            table = g.s444 ? (i % 3 != 0) : (k >= 4);
            nbits = code_block<false>(mine, dc_diff, dc_tab[table], ac_tab[table], cur);
        }
        const int incl = wave_inclusive_sum(nbits, lane);
        int total = carry_bits + __shfl(incl, 63, 64);
        if (active) {
            cur.pos = carry_bits + incl - nbits;
            code_block<true>(mine, dc_diff, dc_tab[table], ac_tab[table], cur);
        }
        const bool last = r0 + kRound >= nblk;
        if (last && (total & 7)) {  // the segment ends on a byte boundary, padded with 1-bits
            const int pad = 8 - (total & 7);
            cur.pos = total;
            if (lane == 0) cur.put((1u << pad) - 1u, pad);
            total += pad;
        }
        wave_sync();
        const int nbytes = total >> 3, nwords = (total + 31) >> 5;
        const unsigned tail = bits[nbytes >> 2];  // holds the incomplete byte (if any) carried into the next round
        for (int w0 = 0; w0 < nwords; w0 += 64) {
            const int w = w0 + lane;
            unsigned word = 0;
            if (w < nwords) word = bits[w], bits[w] = 0;
            int ff = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) ff += (w * 4 + t < nbytes) && ((word >> (24 - 8 * t)) & 255u) == 255u;
            if (kWrite) {
                const int incl_ff = wave_inclusive_sum(ff, lane);
                long long p = at + (long long)w * 4 + stuffed + (incl_ff - ff);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (w * 4 + t >= nbytes) break;
                    const unsigned byte = (word >> (24 - 8 * t)) & 255u;
                    if (p < cap) stream[p] = (uint8_t)byte;
                    ++p;
                    if (byte == 255u) {
                        if (p < cap) stream[p] = 0;
                        ++p;
                    }
                }
                stuffed += __shfl(incl_ff, 63, 64);
            } else {
                stuffed += ff;
            }
        }
        wave_sync();
        carry_bits = total & 7;
        if (lane == 0 && carry_bits) bits[0] = ((tail >> (24 - 8 * (nbytes & 3))) & 255u) << 24;
        plain += nbytes;
        if (kWrite) at += nbytes, at += stuffed, stuffed = 0;
        wave_sync();
    }
    if (kWrite) {
        if (iv == g.I - 1 && lane < 2 && at + lane < cap) stream[at + lane] = lane == 0 ? 0xff : 0xd9;
    } else {
        const long long all = wave_sum(stuffed);
        if (lane == 0) sizes[blockIdx.x] = plain + all;
    }
}

// ----------------------------------------------------------------------------------------------------------- scan
// One workgroup: exclusive scan of what every interval puts on the stream (header or RSTn + segment, + EOI after a
// frame's last one) -> offsets[interval], frame_offsets[F + 1]; status[0] |= 1 when the stream needs more than `cap`.
__global__ __launch_bounds__(1024) void jpeg_scan_kernel(int F, int I, int header_bytes, const long long *__restrict__ sizes,
                                                         long long *__restrict__ offsets,
                                                         long long *__restrict__ frame_offsets, long long cap,
                                                         int *__restrict__ status) {
    __shared__ long long wave_tot[16];
    __shared__ long long carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = (long long)F * I;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long i0 = 0; i0 < n; i0 += 1024) {
        const long long i = i0 + threadIdx.x;
        const int iv = (int)(i % I);
        long long span = 0;
        if (i < n) span = sizes[i] + (iv == 0 ? header_bytes : 2) + (iv == I - 1 ? 2 : 0);
        const long long incl = wave_inclusive_sum(span, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        long long before = carry;
        for (int w = 0; w < wave; ++w) before += wave_tot[w];
        if (i < n) {
            offsets[i] = before + incl - span;
            if (iv == 0) frame_offsets[i / I] = before + incl - span;
        }
        __syncthreads();  // carry and wave_tot have been read
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        frame_offsets[F] = carry;
        if (carry > cap) atomicOr(status, 1);
    }
}

// ----------------------------------------------------------------------------------------------------------- host
static bool make_geom(int F, int H, int W, int subsampling, int restart_rows, Geom &g) {
    if (F <= 0 || H < 1 || W < 1 || H > 65535 || W > 65535 || restart_rows < 0) return false;
    if (subsampling != AMAV_JPEG_420 && subsampling != AMAV_JPEG_444) return false;
    g.F = F, g.H = H, g.W = W;
    g.s444 = subsampling == AMAV_JPEG_444;
    const int mcu = g.s444 ? 8 : 16;
    g.mcux = (W + mcu - 1) / mcu, g.mcuy = (H + mcu - 1) / mcu;
    g.bpm = g.s444 ? 3 : 6;
    g.bpf = g.mcux * g.mcuy * g.bpm;  // <= 8192^2 * 3
    g.gx = (W + 15) / 16, g.T = g.gx * ((H + 15) / 16);
    g.rr = restart_rows == 0 ? g.mcuy : std::min(restart_rows, g.mcuy);
    g.I = (g.mcuy + g.rr - 1) / g.rr;
    if (restart_rows != 0 && (long long)g.rr * g.mcux > 65535) return false;  // DRI counts MCUs in 16 bits
    if ((long long)F * g.bpf > 0x7fffffffLL) return false;                     // block and interval indices stay in int32
    return true;
}

static void scaled_tables(int quality, QuantTables &qt) {  // libjpeg's jpeg_quality_scaling + jpeg_add_quant_table
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) qt.q[t][i] = (uint8_t)std::min(std::max((kQuantBase[t][i] * s + 50) / 100, 1), 255);
}

// SOI .. SOS of every frame of the call
static int build_header(const Geom &g, const QuantTables &qt, bool restarts, uint8_t *out) {
    int n = 0;
    auto put = [&](std::initializer_list<int> bytes) {
        for (int v : bytes) out[n++] = (uint8_t)v;
    };
    put({0xff, 0xd8});
    put({0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xdb, 0, 67, t});
        for (int k = 0; k < 64; ++k) out[n++] = qt.q[t][kZigzag[k]];
    }
    put({0xff, 0xc0, 0, 17, 8, g.H >> 8, g.H & 255, g.W >> 8, g.W & 255, 3, 1, g.s444 ? 0x11 : 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xc4, 0, 2 + 1 + 16 + 12, t});
        for (int i = 0; i < 16; ++i) out[n++] = kDcBits[t][i];
        for (int i = 0; i < 12; ++i) out[n++] = kDcVals[i];
        put({0xff, 0xc4, 0, 2 + 1 + 16 + 162, 0x10 | t});
        for (int i = 0; i < 16; ++i) out[n++] = kAcBits[t][i];
        for (int i = 0; i < 162; ++i) out[n++] = kAcVals[t][i];
    }
    if (restarts) {
        const int mcus = g.rr * g.mcux;
        put({0xff, 0xdd, 0, 4, mcus >> 8, mcus & 255});
    }
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return n;
}

struct Workspace {
    short *const_levels, *levels;
    long long *sizes, *offsets;
    size_t bytes;
};
static Workspace carve(const Geom &g, void *base) {
    Carver c(base);
    Workspace w;
    w.const_levels = c.take<short>(3 * 64);
    w.levels = c.take<short>((size_t)g.F * g.bpf * 64);
    w.sizes = c.take<long long>((size_t)g.F * g.I);
    w.offsets = c.take<long long>((size_t)g.F * g.I);
    w.bytes = c.total();
    return w;
}

// stage (a): levels of every block; const_levels (3 x 64 shorts, device) is needed with a hint only
static void launch_transform(const Geom &g, const void *frames, int rgba_f32, const QuantTables &qt, const int32_t *hint,
                            const float *bg3, short *const_levels, short *levels, hipStream_t stream) {
    const long long total = (long long)g.F * g.bpf;
    const unsigned grid = (unsigned)((total + 31) / 32);
    float bg[3] = {255.f, 255.f, 255.f};
    if (hint) {
        for (int c = 0; c < 3; ++c) bg[c] = (float)quant8(bg3[c]);
        jpeg_transform_kernel<uint8_t, true><<<1, 256, 0, stream>>>(g, nullptr, qt, nullptr, bg[0], bg[1], bg[2], nullptr,
                                                                   const_levels, 3);
    }
    if (rgba_f32)
        jpeg_transform_kernel<float4, false><<<grid, 256, 0, stream>>>(g, static_cast<const float4 *>(frames), qt, hint, bg[0],
                                                                       bg[1], bg[2], const_levels, levels, total);
    else
        jpeg_transform_kernel<uint8_t, false><<<grid, 256, 0, stream>>>(g, static_cast<const uint8_t *>(frames), qt, hint,
                                                                        bg[0], bg[1], bg[2], const_levels, levels, total);
}

}  // namespace jpeg
}  // namespace amav

using namespace amav;
using namespace amav::jpeg;

extern "C" size_t amav_jpeg_stream_bound(int F, int H, int W, int subsampling, int restart_rows) {
    Geom g;
    if (!make_geom(F, H, W, subsampling, restart_rows, g)) return 0;
    // per frame: header, every block at its worst with every byte stuffed, a padded byte and a marker per interval, EOI
    const size_t frame = (size_t)kHeaderMax + 2 * ((size_t)kMaxBlockBytes * g.bpf + g.I) + 2 * (size_t)g.I + 2;
    return frame * (size_t)F;
}

extern "C" size_t amav_jpeg_workspace_bytes(int F, int H, int W, int subsampling, int restart_rows) {
    Geom g;
    if (!make_geom(F, H, W, subsampling, restart_rows, g)) return 0;
    return carve(g, nullptr).bytes;
}

extern "C" int64_t amav_jpeg_num_blocks(int F, int H, int W, int subsampling) {
    Geom g;
    if (!make_geom(F, H, W, subsampling, 0, g)) return 0;
    return (int64_t)F * g.bpf;
}

static int check_common(const char *who, int F, int H, int W, const void *frames, int quality, int subsampling,
                        int restart_rows, const int32_t *hint, const float *bg3, Geom &g) {
    AMAV_REQUIRE(quality >= 1 && quality <= 100, "%s: quality %d outside 1..100", who, quality);
    AMAV_REQUIRE(subsampling == AMAV_JPEG_420 || subsampling == AMAV_JPEG_444, "%s: unknown subsampling %d (420 or 444)",
                 who, subsampling);
    AMAV_REQUIRE(F > 0 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s: sizes outside 1..65535 (F=%d H=%d W=%d)", who,
                 F, H, W);
    AMAV_REQUIRE(restart_rows >= 0, "%s: restart_rows %d is negative", who, restart_rows);
    AMAV_REQUIRE(make_geom(F, H, W, subsampling, restart_rows, g),
                 "%s: %d frames of %dx%d with %d MCU rows per restart interval exceed the encoder's limits", who, F, W, H,
                 restart_rows);
    AMAV_REQUIRE(frames, "%s: NULL frames", who);
    AMAV_REQUIRE(!hint || bg3, "%s: a tile hint needs the background colour", who);
    return AMAV_OK;
}

extern "C" int amav_jpeg_coefficients(int F, int H, int W, const void *frames, int frames_are_rgba_f32, int quality,
                                      int subsampling, const int32_t *tile_hint, const float *bg_host3, void *levels,
                                      size_t levels_bytes, void *workspace, size_t workspace_bytes, void *stream_) {
    Geom g;
    if (int rc = check_common("amav_jpeg_coefficients", F, H, W, frames, quality, subsampling, 0, tile_hint, bg_host3, g))
        return rc;
    AMAV_REQUIRE(levels, "amav_jpeg_coefficients: NULL levels");
    AMAV_REQUIRE(!frames_are_rgba_f32 || (reinterpret_cast<uintptr_t>(frames) & 15) == 0, "amav_jpeg_coefficients: misaligned frames");
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(levels) & 15) == 0, "amav_jpeg_coefficients: misaligned levels");
    const size_t need = (size_t)F * g.bpf * 64 * sizeof(short);
    if (levels_bytes < need) return fail(AMAV_ERR_WORKSPACE, "amav_jpeg_coefficients: levels buffer %zu < %zu", levels_bytes, need);
    if (tile_hint && (!workspace || workspace_bytes < AMAV_JPEG_HINT_WORKSPACE || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return fail(AMAV_ERR_WORKSPACE, "amav_jpeg_coefficients: a tile hint needs a 16-byte aligned workspace of %d bytes (got %zu)",
                    AMAV_JPEG_HINT_WORKSPACE, workspace_bytes);
    QuantTables qt;
    scaled_tables(quality, qt);
    launch_transform(g, frames, frames_are_rgba_f32, qt, tile_hint, bg_host3, static_cast<short *>(workspace),
                     static_cast<short *>(levels), static_cast<hipStream_t>(stream_));
    return check_launch("amav_jpeg_coefficients");
}

extern "C" int amav_jpeg_encode(int F, int H, int W, const void *frames, int frames_are_rgba_f32, int quality,
                                int subsampling, int restart_rows, const int32_t *tile_hint, const float *bg_host3,
                                uint8_t *stream_out, int64_t capacity, int64_t *frame_offsets, int32_t *status,
                                void *workspace, size_t workspace_bytes, void *stream_) {
    Geom g;
    if (int rc = check_common("amav_jpeg_encode", F, H, W, frames, quality, subsampling, restart_rows, tile_hint, bg_host3, g))
        return rc;
    AMAV_REQUIRE(stream_out && frame_offsets && status && capacity >= 0, "amav_jpeg_encode: NULL output pointer or negative capacity");
    AMAV_REQUIRE(!frames_are_rgba_f32 || (reinterpret_cast<uintptr_t>(frames) & 15) == 0, "amav_jpeg_encode: misaligned frames");
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(frame_offsets) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "amav_jpeg_encode: misaligned frame_offsets or status");
    const Workspace ws = carve(g, workspace);
    if (int rc = check_workspace("amav_jpeg_encode", ws.bytes, workspace, workspace_bytes)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    QuantTables qt;
    scaled_tables(quality, qt);
    HeaderBytes hb;
    std::memset(hb.b, 0, sizeof(hb.b));
    const int header_bytes = build_header(g, qt, restart_rows != 0, hb.b);
    launch_transform(g, frames, frames_are_rgba_f32, qt, tile_hint, bg_host3, ws.const_levels, ws.levels, stream);
    const unsigned intervals = (unsigned)(g.F * g.I);
    jpeg_entropy_kernel<false><<<intervals, 64, 0, stream>>>(g, ws.levels, ws.sizes, nullptr, hb, 0, nullptr, 0);
    jpeg_scan_kernel<<<1, 1024, 0, stream>>>(g.F, g.I, header_bytes, ws.sizes, ws.offsets,
                                             reinterpret_cast<long long *>(frame_offsets), (long long)capacity, status);
    jpeg_entropy_kernel<true><<<intervals, 64, 0, stream>>>(g, ws.levels, nullptr, ws.offsets, hb, header_bytes,
                                                            stream_out, (long long)capacity);
    return check_launch("amav_jpeg_encode");
}
