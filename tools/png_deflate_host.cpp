// The device deflate (csrc/png_deflate_core.h) compiled for the host, its 64 lanes run one after the other: a stand-alone
// program for sanitizer builds (tests/test_png_encode_deflate_host.py builds it with -fsanitize=address,undefined) and the
// source of the bytes the GPU must reproduce (tests/test_png_encode_deflate_gpu.py).
//
//   png_deflate_host IN OUT
// IN:  int32 count, then per stream int32 wrapper, int32 modes (1 stored | 2 fixed | 4 dynamic may be chosen; 7 is what
//      the library uses; | 8: no matching, every byte a literal, so that the histogram that is coded is the input's own),
//      int64 capacity, int64 bytes, the bytes.
// OUT: per stream int32 status (2 = AMAV_PNG_STATUS_SIZE), int64 needed, int64 written = min(needed, capacity), the
//      written bytes.
// The pieces are run twice as on the device: once to size them, once to write at the prefix-summed offsets.  Every input
// and every output lives in a heap block of exactly its size, the output at an odd address inside it, so a read past the
// input or a write at or past the capacity is an AddressSanitizer report.  The write is repeated into a buffer with
// guard bytes behind the capacity, which must survive, and both runs must agree.
//
//   png_deflate_host --lengths IN OUT
// build_lengths alone, on histograms the caller chooses (the length limiter's test).  IN: int32 count, then per case
// int32 n (<= 288), int32 limit, n uint32 frequencies.  OUT: per case the n code lengths, one byte each.
#define AMAV_DEFLATE_HOST
#include "../audio-motion-avatar_amd/csrc/png_deflate_core.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace df = amav::deflate;

template <typename T>
static bool get(FILE *f, T &v) {
    return fread(&v, sizeof(T), 1, f) == 1;
}

static void write_pieces(const uint8_t *in, int64_t bytes, int wrapper, int modes, const std::vector<long long> &offset, uint32_t adler,
                         uint8_t *dst, int64_t capacity, df::Lds *lds, int fill) {
    const long long pieces = df::pieces_of(bytes);
    for (long long k = 0; k < pieces; ++k) {
        memset(lds, fill, sizeof(*lds));  // nothing may depend on what an earlier piece left
        uint32_t s1, s2;
        const long long room = capacity - offset[k] > 0 ? capacity - offset[k] : 0;
        df::encode_piece(in + k * df::kPiece, df::piece_len(bytes, k), df::piece_flags(pieces, k, wrapper != 0, false), modes, adler, lds,
                         dst + (room > 0 ? offset[k] : 0), room, &s1, &s2);
    }
}

static int lengths_main(const char *src, const char *dst) {
    FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
    if (!in || !out) return 2;
    int32_t count = 0;
    if (!get(in, count)) return 2;
    df::Lds *lds = new df::Lds;
    for (int32_t c = 0; c < count; ++c) {
        int32_t n, limit;
        if (!get(in, n) || !get(in, limit) || n < 1 || n > df::kLit || limit < 1 || limit > 15) return 2;
        uint32_t *freq = static_cast<uint32_t *>(malloc(n * sizeof(uint32_t)));  // exactly n: a read past it is a report
        uint8_t *lens = static_cast<uint8_t *>(malloc(n));
        if (fread(freq, sizeof(uint32_t), n, in) != (size_t)n) return 2;
        memset(lds, 0xa5, sizeof(*lds));
        df::build_lengths(lds, freq, n, limit, lens);
        fwrite(lens, 1, n, out);
        free(freq), free(lens);
    }
    delete lds;
    fclose(in), fclose(out);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && strcmp(argv[1], "--lengths") == 0) return lengths_main(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t count = 0;
    if (!get(in, count)) return 2;
    df::Lds *lds = new df::Lds;
    for (int32_t n = 0; n < count; ++n) {
        int32_t wrapper, modes;
        int64_t capacity, bytes;
        if (!get(in, wrapper) || !get(in, modes) || !get(in, capacity) || !get(in, bytes)) return 2;
        uint8_t *data = static_cast<uint8_t *>(malloc(bytes ? bytes : 1));
        if (bytes && fread(data, 1, bytes, in) != (size_t)bytes) return 2;
        const long long pieces = df::pieces_of(bytes);
        std::vector<int32_t> piece_bytes(pieces);
        std::vector<uint32_t> s1(pieces), s2(pieces);
        std::vector<long long> offset(pieces);
        for (long long k = 0; k < pieces; ++k) {
            memset(lds, 0xa5, sizeof(*lds));
            piece_bytes[k] = df::encode_piece(data + k * df::kPiece, df::piece_len(bytes, k), df::piece_flags(pieces, k, wrapper != 0, false),
                                              modes, 0, lds, nullptr, 0, &s1[k], &s2[k]);
        }
        uint32_t adler = 0;
        const int64_t needed = df::layout_stream(bytes, pieces, piece_bytes.data(), s1.data(), s2.data(), 0, offset.data(), &adler);
        const int32_t status = needed > capacity ? 2 : 0;
        const int64_t written = needed < capacity ? needed : capacity;
        const int shift = 1 + n % 15;
        uint8_t *block = static_cast<uint8_t *>(malloc(capacity + shift));
        uint8_t *dst = block + shift;  // ends where the block ends
        write_pieces(data, bytes, wrapper, modes, offset, adler, dst, capacity, lds, 0x5a);
        const int kGuard = 64;
        uint8_t *guarded = static_cast<uint8_t *>(malloc(capacity + kGuard));
        memset(guarded, 0xc3, capacity + kGuard);
        write_pieces(data, bytes, wrapper, modes, offset, adler, guarded, capacity, lds, 0xa5);
        for (int g = 0; g < kGuard; ++g)
            if (guarded[capacity + g] != 0xc3) {
                fprintf(stderr, "stream %d: guard byte %d behind the capacity was written\n", n, g);
                return 3;
            }
        if (memcmp(dst, guarded, (size_t)written) != 0) {
            fprintf(stderr, "stream %d: two runs differ\n", n);
            return 3;
        }
        fwrite(&status, sizeof(status), 1, out);
        fwrite(&needed, sizeof(needed), 1, out);
        fwrite(&written, sizeof(written), 1, out);
        fwrite(dst, 1, (size_t)written, out);
        free(data), free(block), free(guarded);
    }
    delete lds;
    fclose(in), fclose(out);
    return 0;
}
