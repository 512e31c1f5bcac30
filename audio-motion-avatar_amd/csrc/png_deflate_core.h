// DEFLATE (RFC 1951) encoder for one wave and one piece of input: LZ77 matching over an LDS hash of 3-byte prefixes, the
// greedy parse, literal/length and distance histograms, length-limited canonical codes, the run-length coded dynamic
// header, the choice between stored, fixed and dynamic coding by exact size, bit emission, Adler-32 partial sums and the
// CRC-32 of a PNG chunk.  png_encode.hip runs it with one wave per piece; a host program that defines AMAV_DEFLATE_HOST
// before including this file gets the same code with the 64 lanes run one after the other and must produce the same
// bytes: between two AMAV_WAVE_SYNCs no lane reads what another lane writes.  The only writes that meet in one LDS word
// in the same step are integer max / add / or (AMAV_LDS_MAX / _ADD / _OR), whose result does not depend on the order.
//
// A stream is cut into pieces of kPiece input bytes.  Every piece is coded without a reference across its start and ends
// on a byte boundary (a stored piece by construction, a Huffman piece with an empty stored block; the last piece carries
// BFINAL instead), so the pieces, laid back to back, are one DEFLATE stream.
//
// Everything outside an AMAV_EACH_LANE block is wave-uniform.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef AMAV_DEFLATE_HOST
#define AMAV_DEFLATE_FN inline
#define AMAV_DEFLATE_BOTH inline
#define AMAV_LDS_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define AMAV_LDS_ADD(p, v) (*(p) += (v))
#define AMAV_LDS_OR(p, v) (*(p) |= (v))
#ifndef AMAV_EACH_LANE
#define AMAV_EACH_LANE(lane) for (int lane = 0; lane < 64; ++lane)
#define AMAV_WAVE_SYNC() ((void)0)
#define AMAV_UNIFORM(x) ((uint32_t)(x))
#endif
#else
#define AMAV_DEFLATE_FN __device__ inline
#define AMAV_DEFLATE_BOTH __host__ __device__ inline  // sizes the launching code needs too
#define AMAV_LDS_MAX(p, v) atomicMax((p), (v))
#define AMAV_LDS_ADD(p, v) atomicAdd((p), (v))
#define AMAV_LDS_OR(p, v) atomicOr((p), (v))
#ifndef AMAV_EACH_LANE
#define AMAV_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define AMAV_EACH_LANE(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define AMAV_WAVE_SYNC()                                          \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)
#endif
#endif

// Diagnostic builds (png_encode.hip under -DAMAV_PNG_STAMPS) define these before including this file; otherwise nothing.
#ifndef AMAV_STAMP
#define AMAV_STAMP_BEGIN
#define AMAV_STAMP(k)
#endif

namespace amav {
namespace deflate {

constexpr int kPiece = 8192;  // AMAV_DEFLATE_PIECE: input bytes per piece
constexpr int kHashBits = 12;
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr int kFarThree = 4096;     // a 3-byte match farther away than this costs more than its literals
constexpr int kStageBytes = 16384;  // one piece's output is staged in LDS; the largest is a forced fixed piece, 9 bits a byte
constexpr int kModeStored = 1, kModeFixed = 2, kModeDynamic = 4, kModeAny = 7;
constexpr int kModeNoMatch = 8;  // tests only: every byte a literal, so the coded histogram is the byte histogram
// what surrounds the piece's DEFLATE bytes
constexpr int kFlagLast = 1;   // the stream's last piece: BFINAL, no empty stored block behind it
constexpr int kFlagHead = 2;   // the zlib header 78 01 goes in front (first piece of a wrapped stream)
constexpr int kFlagTail = 4;   // the Adler-32 goes behind (last piece of a wrapped stream)
constexpr int kFlagIdat = 8;   // the whole is one PNG IDAT chunk: length, type, data, CRC-32
constexpr uint32_t kAdlerMod = 65521u, kCrcPoly = 0xEDB88320u;
constexpr int kLit = 288, kSyms = 320;  // lens / code / freq: 0..287 literal/length, 288..319 distance

struct Lds {  // about 52.5 KB: three waves share a compute unit's 160 KB
    union {  // the piece, as bytes and as little-endian words
        alignas(16) uint8_t buf[kPiece + 16];
        uint32_t bufw[kPiece / 4 + 4];
    };
    uint8_t mlen[kPiece];                 // match length - 3 at a position
    uint16_t mdist[kPiece];               // its distance, 0 = none
    union {
        uint32_t head[1 << kHashBits];     // newest position + 1 with this hash, 0 = none
        uint32_t stage[kStageBytes / 4];   // the output, once the matches are found
        struct {                           // between the two: sort scratch of build_lengths
            uint32_t key[kLit];            // frequency by rank
            uint16_t sym[kLit];            // symbol by rank
        };
    };
    uint32_t vis[kPiece / 32];  // positions at which the greedy parse starts a token
    uint32_t freq[kSyms];
    uint8_t lens[kSyms];
    uint16_t code[kSyms];  // bit-reversed: ready for the LSB-first stream
    uint32_t cl_freq[19];
    uint8_t cl_lens[19];
    uint16_t cl_code[19];
    uint16_t cl_seq[kSyms];  // the header's code-length symbols: symbol | extra value << 8
    uint32_t lane_a[64], lane_b[64];
    uint32_t sc[16];  // what lane 0 hands to the wave
};
enum { kStampMatch, kStampHist, kStampCodes, kStampEmit, kStamps };  // load, matches and parse; histograms; codes and choice; emission
enum { kScMode, kScBits, kScHeaderBits, kScSeq, kScHlit, kScHdist, kScHclen, kScS1, kScS2, kScCrc };

AMAV_DEFLATE_FN int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }
// RFC 1951 3.2.5 turned round: length 3..258 -> code 257 + s with `eb` extra bits of value `ev`; likewise distances.
AMAV_DEFLATE_FN int len_sym(int len, int &eb, int &ev) {
    const int l = len - 3;
    eb = 0, ev = 0;
    if (l < 8) return l;
    if (len == 258) return 28;
    eb = ilog2((uint32_t)l) - 2, ev = l & ((1 << eb) - 1);
    return 4 * (eb + 1) + ((l >> eb) & 3);
}
AMAV_DEFLATE_FN int dist_sym(int dist, int &eb, int &ev) {
    const int d = dist - 1;
    eb = 0, ev = 0;
    if (d < 4) return d;
    eb = ilog2((uint32_t)d) - 1, ev = d & ((1 << eb) - 1);
    return 2 * (eb + 1) + ((d >> eb) & 1);
}
AMAV_DEFLATE_FN int len_extra(int s) { return s < 8 || s >= 28 ? 0 : (s - 4) >> 2; }
AMAV_DEFLATE_FN int dist_extra(int d) { return d < 4 ? 0 : (d - 2) >> 1; }
AMAV_DEFLATE_FN int cl_order(int i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1); }
AMAV_DEFLATE_FN int fixed_len(int i) { return i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8; }
AMAV_DEFLATE_FN int fixed_code(int i) { return i < 144 ? 0x30 + i : i < 256 ? 0x190 + i - 144 : i < 280 ? i - 256 : 0xC0 + i - 280; }
AMAV_DEFLATE_FN unsigned reverse_bits(unsigned c, int len) {
    unsigned r = 0;
    for (int b = 0; b < len; ++b) r |= ((c >> b) & 1u) << (len - 1 - b);
    return r;
}
AMAV_DEFLATE_FN uint32_t hash3(const uint8_t *b) {
    return (((uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16) * 0x9E3779B1u) >> (32 - kHashBits);
}

// bytes o .. o + 3 of the piece as one word, from the two aligned words that hold them
AMAV_DEFLATE_FN uint32_t word_at(const Lds *L, int o) {
    const int i = o >> 2, s = (o & 3) * 8;
    return (uint32_t)((((uint64_t)L->bufw[i + 1] << 32) | L->bufw[i]) >> s);
}
// how many of the bytes at a and at p agree, up to maxlen; four at a time
AMAV_DEFLATE_FN int match_len(const Lds *L, int a, int p, int maxlen) {
    int l = 0;
    while (l < maxlen) {
        const uint32_t x = word_at(L, a + l) ^ word_at(L, p + l);
        if (x) {
            l += __builtin_ctz(x) >> 3;
            break;
        }
        l += 4;
    }
    return l < maxlen ? l : maxlen;
}

// `nb` <= 48 bits of `v` into the staged output at bit `pos` (LSB first).  An OR: the neighbours' bits in the same word
// may arrive before or after.
AMAV_DEFLATE_FN void put_bits(Lds *L, long long pos, uint64_t v, int nb) {
    if (nb == 0) return;
    const int w = (int)(pos >> 5), sh = (int)(pos & 31);
    const uint32_t w0 = (uint32_t)(v << sh);
    const uint64_t rest = (v >> 1) >> (31 - sh);
    if (w0) AMAV_LDS_OR(&L->stage[w], w0);
    if ((uint32_t)rest) AMAV_LDS_OR(&L->stage[w + 1], (uint32_t)rest);
    if ((uint32_t)(rest >> 32)) AMAV_LDS_OR(&L->stage[w + 2], (uint32_t)(rest >> 32));
}

// The token that starts at p under the codes in L->lens / L->code: its bits and their number.
AMAV_DEFLATE_FN int token_bits(const Lds *L, int p, uint64_t &bits) {
    const int d = L->mdist[p];
    if (!d) {
        const int s = L->buf[p];
        bits = L->code[s];
        return L->lens[s];
    }
    int eb, ev;
    const int s = 257 + len_sym(L->mlen[p] + 3, eb, ev);
    uint64_t v = L->code[s];
    int nb = L->lens[s];
    v |= (uint64_t)ev << nb, nb += eb;
    const int ds = kLit + dist_sym(d, eb, ev);
    v |= (uint64_t)L->code[ds] << nb, nb += L->lens[ds];
    v |= (uint64_t)ev << nb, nb += eb;
    bits = v;
    return nb;
}

// Code lengths of at most `limit` bits for the n symbols of `freq`, into lens[0, n).  The lanes rank the used symbols by
// (frequency, symbol); lane 0 runs the in-place minimum-redundancy construction of Moffat and Katajainen over the sorted
// frequencies (two passes, linear), moves the codes deeper than `limit` up until the Kraft sum is exactly one, and hands
// the lengths out shortest to most frequent.  One used symbol gets one bit, none gets nothing.
AMAV_DEFLATE_FN void build_lengths(Lds *L, const uint32_t *freq, int n, int limit, uint8_t *lens) {
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        for (int i = lane; i < n; i += 64) {
            const uint32_t f = freq[i];
            lens[i] = 0;
            if (!f) continue;
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t g = freq[j];
                rank += g && (g < f || (g == f && j < i));
            }
            L->key[rank] = f, L->sym[rank] = (uint16_t)i;
        }
    }
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        if (lane == 0) {
            int used = 0;
            for (int i = 0; i < n; ++i) used += freq[i] != 0;
            uint32_t *A = L->key;
            if (used == 1) {
                lens[L->sym[0]] = 1;
            } else if (used >= 2) {
                A[0] += A[1];
                int root = 0, leaf = 2;
                for (int next = 1; next < used - 1; ++next) {
                    if (leaf >= used || A[root] < A[leaf]) {
                        A[next] = A[root];
                        A[root++] = (uint32_t)next;
                    } else {
                        A[next] = A[leaf++];
                    }
                    if (leaf >= used || (root < next && A[root] < A[leaf])) {
                        A[next] += A[root];
                        A[root++] = (uint32_t)next;
                    } else {
                        A[next] += A[leaf++];
                    }
                }
                A[used - 2] = 0;
                for (int next = used - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
                int avbl = 1, taken = 0, depth = 0, next = used - 1;
                root = used - 2;
                while (avbl > 0) {
                    while (root >= 0 && (int)A[root] == depth) ++taken, --root;
                    while (avbl > taken) A[next--] = (uint32_t)depth, --avbl;
                    avbl = 2 * taken, ++depth, taken = 0;
                }
                // A[r] is now the depth of the symbol of rank r: deepest first
                int count[33];
                for (int i = 0; i <= 32; ++i) count[i] = 0;
                for (int r = 0; r < used; ++r) count[A[r] < 32 ? A[r] : 32]++;
                for (int i = limit + 1; i <= 32; ++i) count[limit] += count[i];
                uint32_t total = 0;
                for (int i = limit; i > 0; --i) total += (uint32_t)count[i] << (limit - i);
                while (total != (1u << limit)) {  // over-subscribed by the clamp: one deepest code less, one leaf split
                    count[limit]--;
                    for (int i = limit - 1; i > 0; --i)
                        if (count[i]) {
                            count[i]--;
                            count[i + 1] += 2;
                            break;
                        }
                    total--;
                }
                int r = used;
                for (int len = 1; len <= limit; ++len)
                    for (int c = count[len]; c > 0; --c) lens[L->sym[--r]] = (uint8_t)len;
            }
        }
    }
    AMAV_WAVE_SYNC();
}

// canonical codes (RFC 1951 3.2.2) of lens[0, n), bit-reversed; run by one lane
AMAV_DEFLATE_FN void assign_codes(const uint8_t *lens, int n, uint16_t *code) {
    int count[16], next[16];
    for (int i = 0; i < 16; ++i) count[i] = 0;
    for (int i = 0; i < n; ++i) count[lens[i]]++;
    count[0] = 0;
    int c = 0;
    for (int len = 1; len < 16; ++len) c = (c + count[len - 1]) << 1, next[len] = c;
    for (int i = 0; i < n; ++i) code[i] = lens[i] ? (uint16_t)reverse_bits((unsigned)next[lens[i]]++, lens[i]) : (uint16_t)0;
}

AMAV_DEFLATE_FN uint32_t crc_mul(uint32_t a, uint32_t b) {  // a x b modulo the CRC-32 polynomial, bit 31 = x^0
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
AMAV_DEFLATE_FN uint32_t crc_xpow(uint32_t bits) {  // x^bits
    uint32_t r = 1u << 31, b = 1u << 30;
    for (; bits; bits >>= 1) {
        if (bits & 1u) r = crc_mul(r, b);
        b = crc_mul(b, b);
    }
    return r;
}

// CRC-32 of the m bytes at `bytes` (LDS): lane k runs the register over the k-th run of ceil(m / 64) bytes, from
// 0xffffffff in lane 0 and from 0 elsewhere (the register is linear in its start value and the data); lane 0 joins them:
// register x x^(8 len) + next.  The result is in L->sc[kScCrc] after the closing sync.
template <typename S>  // S: lane_a[64] and sc[] (Lds, or the few words the container kernel keeps)
AMAV_DEFLATE_FN void crc_wave(S *L, const uint8_t *bytes, int m) {
    const int run = (m + 63) / 64;
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        const int a = lane * run < m ? lane * run : m, b = a + run < m ? a + run : m;
        uint32_t s = lane == 0 ? 0xffffffffu : 0u;
        for (int i = a; i < b; ++i) {
            s ^= bytes[i];
            for (int k = 0; k < 8; ++k) s = (s & 1u) ? (s >> 1) ^ kCrcPoly : s >> 1;
        }
        L->lane_a[lane] = s;
    }
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        if (lane == 0) {
            const uint32_t whole = crc_xpow(8u * (uint32_t)run);
            uint32_t s = L->lane_a[0];
            for (int k = 1; k < 64 && k * run < m; ++k) {
                const int len = (k + 1) * run <= m ? run : m - k * run;
                s = crc_mul(len == run ? whole : crc_xpow(8u * (uint32_t)len), s) ^ L->lane_a[k];
            }
            L->sc[kScCrc] = s ^ 0xffffffffu;
        }
    }
    AMAV_WAVE_SYNC();
}

AMAV_DEFLATE_FN void put_be32(uint8_t *at, uint32_t v) {
    at[0] = (uint8_t)(v >> 24), at[1] = (uint8_t)(v >> 16), at[2] = (uint8_t)(v >> 8), at[3] = (uint8_t)v;
}

// bytes a Huffman block of `bits` bits (3 header bits included) takes with what must follow it
AMAV_DEFLATE_FN long long huffman_bytes(long long bits, bool last) { return last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4; }

// One piece: in[0, n), n <= kPiece.  Returns the bytes it takes with everything `flags` puts around it.  out == nullptr:
// sizing only, and *s1 / *s2 receive the piece's Adler-32 sums (sum of the bytes; sum of (n - i) x byte i; both mod
// 65521).  Otherwise the bytes go to out[0, room) (nothing at or past `room`), with `adler` behind them under kFlagTail.
// `modes`: which of stored / fixed / dynamic may be chosen (kModeAny outside tests; | kModeNoMatch: no matching).
AMAV_DEFLATE_FN int encode_piece(const uint8_t *in, int n, int flags, int modes, uint32_t adler, Lds *L, uint8_t *out, long long room,
                                 uint32_t *s1, uint32_t *s2) {
    const bool last = (flags & kFlagLast) != 0;
    AMAV_STAMP_BEGIN
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        for (int i = lane; i < n; i += 64) L->buf[i] = in[i];  // bounds: i < n
        if (lane < 16) L->buf[n + lane] = 0;  // match_len reads whole words: up to 8 bytes past the piece
        for (int k = lane; k < (1 << kHashBits); k += 64) L->head[k] = 0;
        for (int k = lane; k < kPiece / 32; k += 64) L->vis[k] = 0;
        for (int k = lane; k < kSyms; k += 64) L->freq[k] = 0, L->lens[k] = 0, L->code[k] = 0;
    }
    AMAV_WAVE_SYNC();
    // Matches and the greedy parse, 64 consecutive positions a step.  A position looks at the newest earlier-step position
    // with its hash and at the byte before it (runs); the longer wins, the nearer on a tie.  Then the step's positions
    // enter the table: the largest position wins an entry, whichever lane comes first.  In between the parse, wave-uniform,
    // crosses the step: a match is taken where one starts; the step's match starts are a 64-bit mask (kept in `vis` until
    // the token starts replace them), so a stretch of literals costs one count-trailing-zeros.  Positions the parse has
    // already passed (inside a match that was taken) are not searched: nothing will ask for them.
    {
        int pos = 0;
        for (int base = 0; base < n; base += 64) {
            if (pos < base + 64) {
                AMAV_EACH_LANE(lane) {
                    const int p = base + lane;
                    if (p < n && p >= pos) {
                        const int room_here = n - p < kMaxMatch ? n - p : kMaxMatch;
                        int best = 0, dist = 0;
                        if (room_here >= kMinMatch && !(modes & kModeNoMatch)) {
                            // the run first: where it already has every byte there is, nothing is longer or nearer
                            if (p >= 1) best = match_len(L, p - 1, p, room_here), dist = 1;
                            const int c = (int)L->head[hash3(L->buf + p)] - 1;
                            if (best < room_here && c >= 0 && c != p - 1) {
                                const int l = match_len(L, c, p, room_here);
                                if (l > best) best = l, dist = p - c;
                            }
                            if (best < kMinMatch || (best == kMinMatch && dist > kFarThree)) best = 0, dist = 0;
                        }
                        L->mlen[p] = (uint8_t)(best ? best - kMinMatch : 0);
                        L->mdist[p] = (uint16_t)dist;
                        if (dist) AMAV_LDS_OR(&L->vis[p >> 5], 1u << (p & 31));  // for now: where a match starts
                    }
                }
                AMAV_WAVE_SYNC();
                // the parse across this step: the literals up to the next match in one go, then the match
                const uint64_t has = (uint64_t)AMAV_UNIFORM(L->vis[base >> 5]) | (uint64_t)AMAV_UNIFORM(L->vis[(base >> 5) + 1]) << 32;
                const int end = n - base < 64 ? n - base : 64;
                uint64_t seen = 0;
                int o = pos - base;
                while (o < end) {
                    const uint64_t rest = has >> o;
                    const int lits = rest ? (int)__builtin_ctzll(rest) : end - o;
                    if (lits) seen |= (lits >= 64 ? ~0ull : (1ull << lits) - 1ull) << o;
                    o += lits;
                    if (o >= end) break;
                    seen |= 1ull << o;
                    o += (int)AMAV_UNIFORM(L->mlen[base + o]) + kMinMatch;
                }
                pos = base + o;
                AMAV_EACH_LANE(lane) {
                    if (lane == 0) L->vis[base >> 5] = (uint32_t)seen, L->vis[(base >> 5) + 1] = (uint32_t)(seen >> 32);
                }
            }
            AMAV_EACH_LANE(lane) {
                const int p = base + lane;
                if (p + kMinMatch <= n) AMAV_LDS_MAX(&L->head[hash3(L->buf + p)], (uint32_t)(p + 1));
            }
            AMAV_WAVE_SYNC();
        }
    }
    AMAV_WAVE_SYNC();
    AMAV_STAMP(kStampMatch);
    AMAV_EACH_LANE(lane) {
        for (int p = lane; p < n; p += 64) {
            if (!((L->vis[p >> 5] >> (p & 31)) & 1u)) continue;
            const int d = L->mdist[p];
            if (!d) {
                AMAV_LDS_ADD(&L->freq[L->buf[p]], 1u);
            } else {
                int eb, ev;
                AMAV_LDS_ADD(&L->freq[257 + len_sym(L->mlen[p] + 3, eb, ev)], 1u);
                AMAV_LDS_ADD(&L->freq[kLit + dist_sym(d, eb, ev)], 1u);
            }
        }
        if (lane == 0) AMAV_LDS_ADD(&L->freq[256], 1u);
    }
    AMAV_WAVE_SYNC();
    AMAV_STAMP(kStampHist);
    build_lengths(L, L->freq, 286, 15, L->lens);
    build_lengths(L, L->freq + kLit, 30, 15, L->lens + kLit);
    // the dynamic header: HLIT, HDIST, the two length lists as one, run-length coded (RFC 1951 3.2.7)
    AMAV_EACH_LANE(lane) {
        if (lane == 0) {
            int dused = 0, lused = 0;
            for (int d = 0; d < 30; ++d) dused += L->lens[kLit + d] != 0;
            for (int i = 0; i < 286; ++i) lused += L->lens[i] != 0;
            if (dused == 0) L->lens[kLit] = 1;  // no match in the piece: one distance code of one bit, never sent
            int hlit = 286, hdist = 30;
            while (hlit > 257 && !L->lens[hlit - 1]) --hlit;
            while (hdist > 1 && !L->lens[kLit + hdist - 1]) --hdist;
            for (int i = 0; i < 19; ++i) L->cl_freq[i] = 0;
            const int total = hlit + hdist;
            int seq = 0;
            for (int i = 0; i < total;) {
                const int v = L->lens[i < hlit ? i : kLit + i - hlit];
                int run = 1;
                while (i + run < total && L->lens[i + run < hlit ? i + run : kLit + i + run - hlit] == v) ++run;
                i += run;
                if (v == 0) {
                    while (run >= 11) {
                        const int r = run < 138 ? run : 138;
                        L->cl_seq[seq++] = (uint16_t)(18 | (r - 11) << 8), L->cl_freq[18]++, run -= r;
                    }
                    if (run >= 3) L->cl_seq[seq++] = (uint16_t)(17 | (run - 3) << 8), L->cl_freq[17]++, run = 0;
                } else {
                    L->cl_seq[seq++] = (uint16_t)v, L->cl_freq[v]++, --run;
                    while (run >= 3) {
                        const int r = run < 6 ? run : 6;
                        L->cl_seq[seq++] = (uint16_t)(16 | (r - 3) << 8), L->cl_freq[16]++, run -= r;
                    }
                }
                for (; run > 0; --run) L->cl_seq[seq++] = (uint16_t)v, L->cl_freq[v]++;
            }
            L->sc[kScSeq] = (uint32_t)seq, L->sc[kScHlit] = (uint32_t)hlit, L->sc[kScHdist] = (uint32_t)hdist;
            L->sc[kScMode] = lused >= 2 ? 1u : 0u;  // for now: whether a dynamic block can be written at all
        }
    }
    build_lengths(L, L->cl_freq, 19, 7, L->cl_lens);
    AMAV_EACH_LANE(lane) {
        if (lane == 0) {
            assign_codes(L->lens, 286, L->code);
            assign_codes(L->lens + kLit, 30, L->code + kLit);
            assign_codes(L->cl_lens, 19, L->cl_code);
            int hclen = 19, cl_used = 0;
            while (hclen > 4 && !L->cl_lens[cl_order(hclen - 1)]) --hclen;
            for (int i = 0; i < 19; ++i) cl_used += L->cl_lens[i] != 0;
            const int seq = (int)L->sc[kScSeq];
            long long header = 3 + 14 + 3 * hclen;
            for (int i = 0; i < seq; ++i) {
                const int s = L->cl_seq[i] & 255;
                header += L->cl_lens[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
            }
            long long dyn = header, fix = 3;
            for (int i = 0; i < 286; ++i) {
                const long long f = L->freq[i], extra = i > 256 ? len_extra(i - 257) : 0;
                dyn += f * (L->lens[i] + extra), fix += f * (fixed_len(i) + extra);
            }
            for (int d = 0; d < 30; ++d) {
                const long long f = L->freq[kLit + d];
                dyn += f * (L->lens[kLit + d] + dist_extra(d)), fix += f * (5 + dist_extra(d));
            }
            const bool dyn_ok = L->sc[kScMode] != 0 && cl_used >= 2;
            long long best = 1ll << 40;
            int mode = 0;
            if (modes & kModeStored) best = 5 + n, mode = kModeStored;
            if ((modes & kModeFixed) && huffman_bytes(fix, last) < best) best = huffman_bytes(fix, last), mode = kModeFixed;
            if ((modes & kModeDynamic) && dyn_ok && huffman_bytes(dyn, last) < best) best = huffman_bytes(dyn, last), mode = kModeDynamic;
            if (!mode) best = 5 + n, mode = kModeStored;  // nothing allowed fits the piece: stored always does
            L->sc[kScMode] = (uint32_t)mode;
            L->sc[kScBits] = (uint32_t)(mode == kModeFixed ? fix : dyn);
            L->sc[kScHeaderBits] = (uint32_t)(mode == kModeFixed ? 3 : header);
            L->sc[kScHclen] = (uint32_t)hclen;
        }
    }
    AMAV_WAVE_SYNC();
    AMAV_STAMP(kStampCodes);
    const int mode = (int)AMAV_UNIFORM(L->sc[kScMode]);
    const long long block_bits = AMAV_UNIFORM(L->sc[kScBits]);
    const int header_bits = (int)AMAV_UNIFORM(L->sc[kScHeaderBits]);
    const int body = mode == kModeStored ? 5 + n : (int)huffman_bytes(block_bits, last);
    const int prefix = ((flags & kFlagIdat) ? 8 : 0) + ((flags & kFlagHead) ? 2 : 0);
    const int data = ((flags & kFlagHead) ? 2 : 0) + body + ((flags & kFlagTail) ? 4 : 0);  // an IDAT chunk's length field
    const int total = prefix + body + ((flags & kFlagTail) ? 4 : 0) + ((flags & kFlagIdat) ? 4 : 0);
    if (!out) {
        // Adler-32 sums of the piece, lane k over the k-th run of positions
        const int run = (n + 63) / 64;
        AMAV_EACH_LANE(lane) {
            const int a = lane * run < n ? lane * run : n, b = a + run < n ? a + run : n;
            uint64_t sa = 0, sb = 0;
            for (int i = a; i < b; ++i) sa += L->buf[i], sb += (uint64_t)(n - i) * L->buf[i];
            L->lane_a[lane] = (uint32_t)(sa % kAdlerMod), L->lane_b[lane] = (uint32_t)(sb % kAdlerMod);
        }
        AMAV_WAVE_SYNC();
        AMAV_EACH_LANE(lane) {
            if (lane == 0) {
                uint64_t sa = 0, sb = 0;
                for (int k = 0; k < 64; ++k) sa += L->lane_a[k], sb += L->lane_b[k];
                L->sc[kScS1] = (uint32_t)(sa % kAdlerMod), L->sc[kScS2] = (uint32_t)(sb % kAdlerMod);
            }
        }
        AMAV_WAVE_SYNC();
        *s1 = AMAV_UNIFORM(L->sc[kScS1]), *s2 = AMAV_UNIFORM(L->sc[kScS2]);
        return total;
    }

    uint8_t *stage = reinterpret_cast<uint8_t *>(L->stage);
    AMAV_EACH_LANE(lane) {
        if (mode == kModeFixed) {
            for (int i = lane; i < kLit; i += 64) L->lens[i] = (uint8_t)fixed_len(i), L->code[i] = (uint16_t)reverse_bits((unsigned)fixed_code(i), fixed_len(i));
            if (lane < 32) L->lens[kLit + lane] = 5, L->code[kLit + lane] = (uint16_t)reverse_bits((unsigned)lane, 5);
        }
        for (int k = lane; k < (total + 3) / 4 + 3 && k < kStageBytes / 4; k += 64) L->stage[k] = 0;
    }
    AMAV_WAVE_SYNC();
    const long long first_bit = 8ll * prefix;
    AMAV_EACH_LANE(lane) {  // what stands before the tokens
        if (lane == 0) {
            int at = 0;
            if (flags & kFlagIdat) {
                put_be32(stage, (uint32_t)data);
                stage[4] = 'I', stage[5] = 'D', stage[6] = 'A', stage[7] = 'T';
                at = 8;
            }
            if (flags & kFlagHead) stage[at] = 0x78, stage[at + 1] = 0x01;
            if (mode == kModeStored) {
                uint8_t *h = stage + prefix;
                h[0] = last ? 1 : 0, h[1] = (uint8_t)n, h[2] = (uint8_t)(n >> 8), h[3] = (uint8_t)~n, h[4] = (uint8_t)(~n >> 8);
            }
        }
    }
    AMAV_WAVE_SYNC();
    if (mode == kModeStored) {
        AMAV_EACH_LANE(lane) {
            for (int i = lane; i < n; i += 64) stage[prefix + 5 + i] = L->buf[i];
        }
    } else {
        AMAV_EACH_LANE(lane) {
            if (lane == 0) {
                long long pos = first_bit;
                put_bits(L, pos, (last ? 1u : 0u) | (mode == kModeFixed ? 2u : 4u), 3), pos += 3;
                if (mode == kModeDynamic) {
                    const int hclen = (int)L->sc[kScHclen], seq = (int)L->sc[kScSeq];
                    put_bits(L, pos, L->sc[kScHlit] - 257, 5), pos += 5;
                    put_bits(L, pos, L->sc[kScHdist] - 1, 5), pos += 5;
                    put_bits(L, pos, (uint64_t)(hclen - 4), 4), pos += 4;
                    for (int i = 0; i < hclen; ++i) put_bits(L, pos, L->cl_lens[cl_order(i)], 3), pos += 3;
                    for (int i = 0; i < seq; ++i) {
                        const int s = L->cl_seq[i] & 255, extra = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
                        put_bits(L, pos, L->cl_code[s], L->cl_lens[s]), pos += L->cl_lens[s];
                        put_bits(L, pos, (uint64_t)(L->cl_seq[i] >> 8), extra), pos += extra;
                    }
                }
            }
        }
        AMAV_WAVE_SYNC();
        // tokens: lane k owns the k-th run of positions; it counts its bits, learns where it starts, and writes
        const int run = (n + 63) / 64;
        AMAV_EACH_LANE(lane) {
            const int a = lane * run < n ? lane * run : n, b = a + run < n ? a + run : n;
            uint32_t sum = 0;
            for (int p = a; p < b; ++p)
                if ((L->vis[p >> 5] >> (p & 31)) & 1u) {
                    uint64_t v;
                    sum += (uint32_t)token_bits(L, p, v);
                }
            L->lane_a[lane] = sum;
        }
        AMAV_WAVE_SYNC();
        AMAV_EACH_LANE(lane) {
            const int a = lane * run < n ? lane * run : n, b = a + run < n ? a + run : n;
            long long pos = first_bit + header_bits;
            for (int k = 0; k < lane; ++k) pos += L->lane_a[k];
            for (int p = a; p < b; ++p)
                if ((L->vis[p >> 5] >> (p & 31)) & 1u) {
                    uint64_t v;
                    const int nb = token_bits(L, p, v);
                    put_bits(L, pos, v, nb), pos += nb;
                }
            if (lane == 63) put_bits(L, pos, L->code[256], L->lens[256]);  // end of block
        }
    }
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        if (lane == 0) {
            if (mode != kModeStored && !last) {  // the empty stored block: 000, up to the byte boundary, 00 00 ff ff
                uint8_t *m = stage + prefix + body - 4;
                m[2] = 0xff, m[3] = 0xff;
            }
            if (flags & kFlagTail) put_be32(stage + prefix + body, adler);
        }
    }
    if (flags & kFlagIdat) {
        crc_wave(L, stage + 4, 4 + data);
        const uint32_t crc = AMAV_UNIFORM(L->sc[kScCrc]);
        AMAV_EACH_LANE(lane) {
            if (lane == 0) put_be32(stage + 8 + data, crc);
        }
    }
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        for (int i = lane; i < total; i += 64)
            if (i < room) out[i] = stage[i];  // bounds: nothing at or past `room`
    }
    AMAV_WAVE_SYNC();
    AMAV_STAMP(kStampEmit);
    return total;
}

AMAV_DEFLATE_BOTH long long pieces_of(long long bytes) { return bytes <= 0 ? 1 : (bytes + kPiece - 1) / kPiece; }
AMAV_DEFLATE_FN int piece_len(long long bytes, long long k) { return (int)(bytes - k * kPiece < kPiece ? (bytes > 0 ? bytes - k * kPiece : 0) : kPiece); }
AMAV_DEFLATE_FN int piece_flags(long long pieces, long long k, bool wrapper, bool idat) {
    return (k == pieces - 1 ? kFlagLast : 0) | (wrapper && k == 0 ? kFlagHead : 0) | (wrapper && k == pieces - 1 ? kFlagTail : 0) |
           (idat ? kFlagIdat : 0);
}

// One stream's pieces laid back to back from `at`: offset[k] for each, the end, and the Adler-32 of the whole input from
// the pieces' sums: with (a, b) before a piece of n bytes, b += n a + s2, a += s1 (mod 65521).  Run by one thread.
AMAV_DEFLATE_FN long long layout_stream(long long bytes, long long pieces, const int32_t *piece_bytes, const uint32_t *s1, const uint32_t *s2,
                                        long long at, long long *offset, uint32_t *adler) {
    uint64_t a = 1, b = 0;
    for (long long k = 0; k < pieces; ++k) {
        offset[k] = at;
        at += piece_bytes[k];
        b = (b + (uint64_t)piece_len(bytes, k) * a + s2[k]) % kAdlerMod;
        a = (a + s1[k]) % kAdlerMod;
    }
    *adler = (uint32_t)(b << 16 | a);
    return at;
}

}  // namespace deflate
}  // namespace amav
