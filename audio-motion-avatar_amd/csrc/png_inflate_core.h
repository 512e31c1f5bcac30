// DEFLATE (RFC 1951) decoder for one wave: the bit reader, the canonical-code table builder, the symbol decoder and the
// history ring.  png_decode.hip runs it with one wave per stream; a host program that defines AMAV_INFLATE_HOST before
// including this file gets the same code with the 64 lanes run one after the other, so the damaged-stream list can go
// through a sanitizer build on the CPU (the steps between two AMAV_WAVE_SYNCs never have one lane read what another
// lane writes in the same step, so lockstep and lane-after-lane give the same bytes).
//
// Everything outside an AMAV_EACH_LANE block is wave-uniform: every lane computes the same value from the same LDS
// words (broadcast reads).  The lanes differ only where they fill tables, load the input window, copy a match and flush.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef AMAV_INFLATE_HOST
#define AMAV_INFLATE_FN inline
#define AMAV_EACH_LANE(lane) for (int lane = 0; lane < 64; ++lane)
#define AMAV_WAVE_SYNC() ((void)0)
#define AMAV_UNIFORM(x) ((uint32_t)(x))
#else
// a value every lane holds alike (read from one LDS address): telling the compiler so keeps the decoder's state and its
// branches in scalar registers
#define AMAV_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define AMAV_INFLATE_FN __device__ inline
#define AMAV_EACH_LANE(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define AMAV_WAVE_SYNC()                                          \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)
#endif

namespace amav {
namespace inflate {

constexpr int kStatusInflate = 1, kStatusSize = 2;  // AMAV_PNG_STATUS_INFLATE / _SIZE
constexpr int kRing = 32768, kRingMask = kRing - 1;  // the DEFLATE window
constexpr int kWindowBytes = 1024;                   // staged input
constexpr int kLookBits = 10;
constexpr int kFlushAt = 8192, kChunk = 1024;  // pending bytes that trigger a flush; longest single emit (a match is 258)

// RFC 1951 3.2.5 in arithmetic (a table in global memory would put two dependent loads into every match): length code
// 257 + s: s < 8: 3 + s, no extra bits; s = 28: 258; else (s - 4) >> 2 extra bits on 3 + ((4 + (s & 3)) << extra).
// Distance code d: d < 4: 1 + d; else (d - 2) >> 1 extra bits on 1 + ((2 + (d & 1)) << extra).
AMAV_INFLATE_FN int len_extra(int s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
AMAV_INFLATE_FN int len_base(int s) { return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << len_extra(s)); }
AMAV_INFLATE_FN int dist_extra(int d) { return d < 4 ? 0 : (d - 2) >> 1; }
AMAV_INFLATE_FN int dist_base(int d) { return d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << dist_extra(d)); }
// the order in which a dynamic header sends the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
AMAV_INFLATE_FN int cl_order(int i) {
    return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
}

struct alignas(16) Bytes16 {
    uint32_t w[4];
};

// One canonical code: a first-level lookup of the next kLookBits bits (length << 9 | symbol, 0 = longer or unused) and,
// for everything else, the per-length first code / count / offset into the symbols sorted by (length, symbol).
struct alignas(8) LengthInfo {
    uint16_t first, count, offset, pad;  // first code of this length, codes of this length, their place in `sorted`
};
struct HuffTable {
    uint16_t look[1 << kLookBits];
    uint16_t sorted[288];
    LengthInfo len[16];  // one 8-byte read per length on the long-code path
};

struct Lds {  // 40 000 bytes
    alignas(16) uint8_t ring[kRing];
    uint32_t window[kWindowBytes / 4];
    HuffTable lit, dist;  // dist also holds the code-length code while a dynamic header is read
    uint8_t lens[320];
    uint16_t code_of[320];
    uint8_t cl_lens[32];
};

struct State {  // wave-uniform
    const uint8_t *in;
    long long in_pos, in_end, win_base;  // next byte to enter the bit buffer; staged window start (-1: none)
    uint64_t bitbuf;
    int bitcnt;
    uint8_t *out;  // the stream's output: out[0 .. cap)
    long long cap, out_pos, flushed;
    unsigned skew;  // (address of out) & 15: ring index = (position + skew) & kRingMask, so 16-byte units line up
    int status;
};

AMAV_INFLATE_FN void load_window(State &s, Lds *L) {
    s.win_base = s.in_pos;
    AMAV_EACH_LANE(lane) {
        for (int k = lane; k < kWindowBytes / 4; k += 64) {
            uint32_t word = 0;
            for (int b = 0; b < 4; ++b) {
                const long long q = s.win_base + 4 * k + b;
                if (q < s.in_end) word |= (uint32_t)s.in[q] << (8 * b);  // bounds: nothing is read at or past in_end
            }
            L->window[k] = word;
        }
    }
    AMAV_WAVE_SYNC();
}

// After refill() at least 32 bits are in the buffer (32 exactly when it was empty); no consumer takes more between two
// refills: a stored block's LEN + NLEN 32, a distance code with its extra bits 28, a length code with its 20.  Past in_end the window holds zeros: the position keeps counting,
// exhausted() reports it, and the caller stops.
AMAV_INFLATE_FN void refill(State &s, Lds *L) {
    if (s.bitcnt <= 32) {
        if (s.win_base < 0 || s.in_pos - s.win_base >= kWindowBytes) load_window(s, L);  // bounds: in_pos against in_end, in there
        s.bitbuf |= (uint64_t)AMAV_UNIFORM(L->window[(s.in_pos - s.win_base) >> 2]) << s.bitcnt;
        s.bitcnt += 32;
        s.in_pos += 4;
    }
}
AMAV_INFLATE_FN unsigned peek(const State &s, int n) { return (unsigned)(s.bitbuf & ((1ull << n) - 1ull)); }
AMAV_INFLATE_FN void drop(State &s, int n) {
    s.bitbuf >>= n;
    s.bitcnt -= n;
}
AMAV_INFLATE_FN unsigned take(State &s, int n) {
    const unsigned v = peek(s, n);
    drop(s, n);
    return v;
}
// more bits consumed than the stream has
AMAV_INFLATE_FN bool exhausted(const State &s) { return s.in_pos * 8 - s.bitcnt > s.in_end * 8; }

// counts -> prefix -> fill.  false: over-subscribed lengths.  An incomplete set is accepted; its unused codes decode to -1.
AMAV_INFLATE_FN bool build_table(Lds *L, HuffTable &t, const uint8_t *lens, int n) {
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        if (lane < 16) {
            int c = 0;
            for (int i = 0; i < n; ++i) c += (lane != 0 && lens[i] == lane);
            t.len[lane].count = (uint16_t)c;
        }
        for (int k = lane; k < (1 << kLookBits); k += 64) t.look[k] = 0;
    }
    AMAV_WAVE_SYNC();
    int left = 1, code = 0, off = 0;
    bool ok = true;
    for (int len = 1; len <= 15; ++len) {
        const int c = (int)AMAV_UNIFORM(t.len[len].count);
        left = 2 * left - c;
        ok = ok && left >= 0;
        AMAV_EACH_LANE(lane) {
            if (lane == 0) t.len[len].first = (uint16_t)code, t.len[len].offset = (uint16_t)off;
        }
        code = ok ? (code + c) << 1 : 0;
        off += c;
    }
    if (!ok) return false;
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        if (lane >= 1 && lane <= 15) {
            int idx = t.len[lane].offset, c = t.len[lane].first;
            for (int i = 0; i < n; ++i)
                if (lens[i] == lane) {
                    t.sorted[idx++] = (uint16_t)i;
                    L->code_of[i] = (uint16_t)c++;
                }
        }
    }
    AMAV_WAVE_SYNC();
    AMAV_EACH_LANE(lane) {
        for (int i = lane; i < n; i += 64) {
            const int len = lens[i];
            if (len == 0 || len > kLookBits) continue;
            unsigned c = L->code_of[i], rev = 0;
            for (int b = 0; b < len; ++b) rev |= ((c >> b) & 1u) << (len - 1 - b);  // codes are packed starting at the MSB
            for (unsigned k = rev; k < (1u << kLookBits); k += 1u << len) t.look[k] = (uint16_t)(len << 9 | i);
        }
    }
    AMAV_WAVE_SYNC();
    return true;
}

AMAV_INFLATE_FN unsigned reverse15(unsigned v) {  // bit 0 of v -> bit 14
#ifdef AMAV_INFLATE_HOST
    unsigned r = 0;
    for (int b = 0; b < 15; ++b) r |= ((v >> b) & 1u) << (14 - b);
    return r;
#else
    return __brev(v) >> 17;
#endif
}

// The next symbol of code `t`, or -1 (a code not in the set; nothing is consumed then).  Needs 15 bits in the buffer.
// A code of up to kLookBits bits is one lookup.  Otherwise no shorter code matches (it would be in the lookup), so the
// lengths above kLookBits are tried: the first L bits, taken MSB first, are a code of length L exactly when they fall
// into [first, first + count) of that length (a canonical, prefix-free code).
AMAV_INFLATE_FN int decode(State &s, const HuffTable &t) {
    const unsigned e = AMAV_UNIFORM(t.look[peek(s, kLookBits)]);
    if (e) {
        drop(s, (int)(e >> 9));
        return (int)(e & 511u);
    }
    const unsigned rev = reverse15(peek(s, 15));
    for (int len = kLookBits + 1; len <= 15; ++len) {
        const unsigned first = AMAV_UNIFORM(t.len[len].first), count = AMAV_UNIFORM(t.len[len].count);
        const unsigned idx = (rev >> (15 - len)) - first;
        if (idx < count) {
            drop(s, len);
            return (int)AMAV_UNIFORM(t.sorted[AMAV_UNIFORM(t.len[len].offset) + idx]);
        }
    }
    return -1;
}

// Ring -> global: a head of single bytes up to a 16-byte boundary of the output address, whole 16-byte units (coalesced:
// lane u takes unit u), and, at the end of the stream only, the tail of single bytes.
AMAV_INFLATE_FN void flush(State &s, Lds *L, bool final) {
    AMAV_WAVE_SYNC();
    const int mis = (int)((s.flushed + s.skew) & 15);
    if (mis) {
        const long long pending = s.out_pos - s.flushed;
        const int head = (int)(16 - mis < pending ? 16 - mis : pending);
        AMAV_EACH_LANE(lane) {
            const long long p = s.flushed + lane;
            if (lane < head && p < s.cap) s.out[p] = L->ring[(p + s.skew) & kRingMask];  // bounds: store against out_capacity
        }
        s.flushed += head;
    }
    const long long units = (s.out_pos - s.flushed) >> 4;
    AMAV_EACH_LANE(lane) {
        for (long long u = lane; u < units; u += 64) {
            const long long p = s.flushed + 16 * u;
            const Bytes16 v = *reinterpret_cast<const Bytes16 *>(&L->ring[(p + s.skew) & kRingMask]);  // ring index masked
            if (p + 16 <= s.cap) *reinterpret_cast<Bytes16 *>(s.out + p) = v;  // bounds: store against out_capacity
        }
    }
    s.flushed += 16 * units;
    if (final) {
        const int tail = (int)(s.out_pos - s.flushed);  // < 16
        AMAV_EACH_LANE(lane) {
            const long long p = s.flushed + lane;
            if (lane < tail && p < s.cap) s.out[p] = L->ring[(p + s.skew) & kRingMask];  // bounds: store against out_capacity
        }
        s.flushed = s.out_pos;
    }
    AMAV_WAVE_SYNC();
}

// Room for n <= kChunk more bytes: false (and the SIZE bit) if they would pass the capacity; the ring never holds more
// than kFlushAt + kChunk + 15 unflushed bytes, so no unflushed byte is overwritten.
AMAV_INFLATE_FN bool reserve(State &s, Lds *L, int n) {
    if (s.out_pos + n > s.cap) {
        s.status |= kStatusSize;
        return false;
    }
    if (s.out_pos - s.flushed >= kFlushAt) flush(s, L, false);
    return true;
}

AMAV_INFLATE_FN bool bad(State &s) {
    s.status |= kStatusInflate;
    return false;
}

// The code lengths of a dynamic block (RFC 1951 3.2.7) and its two tables.
AMAV_INFLATE_FN bool dynamic_header(State &s, Lds *L) {
    refill(s, L);
    const int hlit = (int)take(s, 5) + 257, hdist = (int)take(s, 5) + 1, hclen = (int)take(s, 4) + 4;
    if (hlit > 286 || hdist > 30) return bad(s);
    AMAV_EACH_LANE(lane) {
        if (lane < 19) L->cl_lens[lane] = 0;
    }
    AMAV_WAVE_SYNC();
    for (int i = 0; i < hclen; ++i) {  // each trip consumes 3 bits
        refill(s, L);
        const unsigned v = take(s, 3);
        AMAV_EACH_LANE(lane) {
            if (lane == 0) L->cl_lens[cl_order(i)] = (uint8_t)v;
        }
    }
    if (exhausted(s)) return bad(s);
    if (!build_table(L, L->dist, L->cl_lens, 19)) return bad(s);
    const int total = hlit + hdist;
    int i = 0, prev = 0;
    while (i < total) {  // each trip consumes at least one bit or ends the stream
        refill(s, L);
        const int sym = decode(s, L->dist);
        if (sym < 0 || exhausted(s)) return bad(s);
        int rep = 1, value = sym;
        if (sym == 16) {
            if (i == 0) return bad(s);  // nothing to repeat
            rep = 3 + (int)take(s, 2), value = prev;
        } else if (sym == 17) {
            rep = 3 + (int)take(s, 3), value = 0;
        } else if (sym == 18) {
            rep = 11 + (int)take(s, 7), value = 0;
        }
        if (i + rep > total) return bad(s);  // a repeat may cross from HLIT into HDIST, not past both
        AMAV_EACH_LANE(lane) {
            for (int k = lane; k < rep; k += 64) L->lens[i + k] = (uint8_t)value;
        }
        i += rep, prev = value;
    }
    if (exhausted(s)) return bad(s);
    if (!build_table(L, L->lit, L->lens, hlit)) return bad(s);
    if (!build_table(L, L->dist, L->lens + hlit, hdist)) return bad(s);
    return true;
}

AMAV_INFLATE_FN bool fixed_tables(State &s, Lds *L) {
    AMAV_EACH_LANE(lane) {
        for (int i = lane; i < 320; i += 64) L->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    }
    return build_table(L, L->lit, L->lens, 288) && build_table(L, L->dist, L->lens + 288, 32);
}

// A stored block's LEN bytes go from the input to the ring without passing the bit buffer.
AMAV_INFLATE_FN bool stored_block(State &s, Lds *L) {
    drop(s, s.bitcnt & 7);
    refill(s, L);
    const unsigned len = take(s, 16), nlen = take(s, 16);
    if (exhausted(s) || (len ^ 0xffffu) != nlen) return bad(s);
    long long src = s.in_pos - s.bitcnt / 8;  // the buffer holds whole bytes here
    s.bitbuf = 0, s.bitcnt = 0, s.win_base = -1;
    if (src + (long long)len > s.in_end) return bad(s);  // bounds: the copy below stays before in_end
    for (unsigned done = 0; done < len;) {
        const int n = (int)(len - done < (unsigned)kChunk ? len - done : (unsigned)kChunk);
        if (!reserve(s, L, n)) return false;
        AMAV_EACH_LANE(lane) {
            for (int i = lane; i < n; i += 64) L->ring[(s.out_pos + s.skew + i) & kRingMask] = s.in[src + i];  // ring index masked
        }
        s.out_pos += n, src += n, done += (unsigned)n;
    }
    s.in_pos = src;
    return true;
}

// The symbols of one Huffman block up to its end-of-block.
AMAV_INFLATE_FN bool huffman_block(State &s, Lds *L) {
    for (;;) {  // each trip consumes at least one bit or ends the stream
        refill(s, L);
        const int sym = decode(s, L->lit);
        if (sym < 0 || exhausted(s)) return bad(s);
        if (sym < 256) {
            if (!reserve(s, L, 1)) return false;
            AMAV_EACH_LANE(lane) {
                if (lane == 0) L->ring[(s.out_pos + s.skew) & kRingMask] = (uint8_t)sym;  // ring index masked
            }
            s.out_pos += 1;
            continue;
        }
        if (sym == 256) return true;
        if (sym >= 286) return bad(s);
        const int len = len_base(sym - 257) + (int)take(s, len_extra(sym - 257));
        refill(s, L);
        const int dsym = decode(s, L->dist);
        if (dsym < 0 || dsym >= 30) return bad(s);
        const long long dist = dist_base(dsym) + (long long)take(s, dist_extra(dsym));
        if (exhausted(s)) return bad(s);
        if (dist > s.out_pos) return bad(s);  // before the start of the output
        if (!reserve(s, L, len)) return false;
        AMAV_WAVE_SYNC();
        // byte i of the match is src[i mod distance]: every source byte lies before out_pos, already in the ring
        const unsigned from = (unsigned)((s.out_pos - dist + s.skew) & kRingMask), to = (unsigned)((s.out_pos + s.skew) & kRingMask);
        const unsigned d = (unsigned)dist, stride = d < 64u ? 64u % d : 64u;
        unsigned base_mod = 0;  // base mod d, kept by additions: the lanes never divide by more than their own index
        for (int base = 0; base < len; base += 64) {  // all lanes read, then all lanes write, 64 bytes at a time
            AMAV_EACH_LANE(lane) {
                const int i = base + lane;
                if (i < len) {
                    unsigned j = (unsigned)i;
                    if (d < (unsigned)len) {
                        j = base_mod + (d <= (unsigned)lane ? (unsigned)lane % d : (unsigned)lane);
                        if (j >= d) j -= d;
                    }
                    const uint8_t v = L->ring[(from + j) & kRingMask];  // ring index masked
                    L->ring[(to + i) & kRingMask] = v;                  // ring index masked
                }
            }
            base_mod += stride;  // < 2 d
            if (base_mod >= d) base_mod -= d;
        }
        AMAV_WAVE_SYNC();
        s.out_pos += len;
    }
}

// One stream: in[in_begin, in_end) -> out[0, cap).  Returns the status bits; *produced = bytes written.
AMAV_INFLATE_FN int inflate_stream(const uint8_t *in, long long in_begin, long long in_end, int wrapper, uint8_t *out, long long cap,
                                   Lds *L, long long *produced) {
    State s;
    s.in = in, s.in_pos = in_begin, s.in_end = in_end, s.win_base = -1, s.bitbuf = 0, s.bitcnt = 0;
    s.out = out, s.cap = cap, s.out_pos = 0, s.flushed = 0, s.skew = (unsigned)(reinterpret_cast<uintptr_t>(out) & 15), s.status = 0;
    bool go = true;
    if (wrapper) {  // RFC 1950: CMF, FLG; the Adler-32 after the last block is neither read nor verified
        if (in_end - in_begin < 2) {
            go = bad(s);
        } else {
            const unsigned cmf = in[in_begin], flg = in[in_begin + 1];
            if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) go = bad(s);  // FDICT refused
            s.in_pos = in_begin + 2;
        }
    }
    bool fixed_built = false;
    while (go) {  // each block consumes at least its 3 header bits
        refill(s, L);
        const unsigned last = take(s, 1), type = take(s, 2);
        if (exhausted(s)) {
            go = bad(s);
        } else if (type == 0) {
            go = stored_block(s, L);
        } else if (type == 1) {
            if (!fixed_built) go = fixed_tables(s, L);
            fixed_built = true;
            go = go && huffman_block(s, L);
        } else if (type == 2) {
            fixed_built = false;
            go = dynamic_header(s, L) && huffman_block(s, L);
        } else {
            go = bad(s);
        }
        if (last) break;
    }
    flush(s, L, true);
    *produced = s.out_pos;
    return s.status;
}

}  // namespace inflate
}  // namespace amav
