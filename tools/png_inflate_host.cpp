// The device inflate (csrc/png_inflate_core.h) compiled for the host, its 64 lanes run one after the other: a stand-alone
// program for sanitizer builds (tests/test_png_inflate_host.py builds it with -fsanitize=address,undefined and sends the
// sound and the damaged stream lists through it before a GPU sees them).
//
//   png_inflate_host IN OUT
// IN:  int32 count, then per stream int32 wrapper, int64 capacity, int64 bytes, the bytes.
// OUT: per stream int32 status, int64 produced, the produced bytes.
// Every stream and every output lives in a heap block of exactly its size, the output at an odd address inside it, so a
// read past in_end or a write past the capacity is an AddressSanitizer report and not a silent pass.
#define AMAV_INFLATE_HOST
#include "../audio-motion-avatar_amd/csrc/png_inflate_core.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

template <typename T>
static bool get(FILE *f, T &v) {
    return fread(&v, sizeof(T), 1, f) == 1;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t count = 0;
    if (!get(in, count)) return 2;
    amav::inflate::Lds *lds = new amav::inflate::Lds;
    for (int32_t n = 0; n < count; ++n) {
        int32_t wrapper;
        int64_t capacity, bytes;
        if (!get(in, wrapper) || !get(in, capacity) || !get(in, bytes)) return 2;
        uint8_t *stream = static_cast<uint8_t *>(malloc(bytes ? bytes : 1));
        if (bytes && fread(stream, 1, bytes, in) != (size_t)bytes) return 2;
        const int shift = 1 + n % 15;  // over the run the output starts at every residue mod 16 but 0; `exact` below has 0
        uint8_t *block = static_cast<uint8_t *>(malloc(capacity + shift));
        uint8_t *dst = block + shift;  // ends where the block ends
        uint8_t *exact = static_cast<uint8_t *>(malloc(capacity ? capacity : 1));  // capacity bytes and no more
        long long produced = 0;
        memset(lds, 0xa5, sizeof(*lds));  // nothing may depend on what an earlier stream left
        // first into the exactly sized block (aligned start), then at the odd address; both must agree
        const int32_t status0 = amav::inflate::inflate_stream(stream, 0, bytes, wrapper, exact, capacity, lds, &produced);
        long long again = 0;
        memset(lds, 0x5a, sizeof(*lds));
        const int32_t status = amav::inflate::inflate_stream(stream, 0, bytes, wrapper, dst, capacity, lds, &again);
        if (status != status0 || produced != again || memcmp(exact, dst, (size_t)produced) != 0) {
            fprintf(stderr, "stream %d: aligned and unaligned outputs differ\n", n);
            return 3;
        }
        const int64_t made = produced;
        fwrite(&status, sizeof(status), 1, out);
        fwrite(&made, sizeof(made), 1, out);
        fwrite(dst, 1, (size_t)made, out);
        free(stream), free(block), free(exact);
    }
    delete lds;
    fclose(in), fclose(out);
    return 0;
}
