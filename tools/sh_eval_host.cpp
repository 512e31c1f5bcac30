// csrc/sh_eval.h on the CPU: the forward and the backward of the spherical-harmonic colours for dense cases read from a
// binary file, so that the polynomials, their derivatives and the clamp gate can be checked (and run under host
// sanitizers) without a GPU.  tests/test_sh_eval_host.py builds and drives it.
//
//   sh_eval_host <in> <out>
//   in : int32 cases, then per case  int32 degree, K, F, N;  float means3d[F*N*3], campos[F*3], sh[F*N*3*K],
//                                     grad_colors[F*N*3]
//   out: per case  float colors[F*N*3], grad_sh[F*N*3*K], grad_means3d[F*N*3]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../audio-motion-avatar_amd/csrc/sh_eval.h"

using namespace amav::sh;

template <int D>
static void run_case(int K, int F, int N, const float *means, const float *campos, const float *sh, const float *grad,
                     float *colors, float *grad_sh, float *grad_means) {
    const int rec = 3 * K;
    for (int f = 0; f < F; ++f)
        for (int n = 0; n < N; ++n) {
            const size_t row = (size_t)f * N + n;
            colour<D>(means + row * 3, campos + (size_t)f * 3, sh + row * rec, colors + row * 3);
            colour_backward<D>(means + row * 3, campos + (size_t)f * 3, sh + row * rec, grad + row * 3, grad_sh + row * rec,
                               grad_means + row * 3, true);
            for (int j = 3 * num_coeffs(D); j < rec; ++j) grad_sh[row * rec + j] = 0.0f;
        }
}

static bool read_all(FILE *fh, void *dst, size_t bytes) { return fread(dst, 1, bytes, fh) == bytes; }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        return 2;
    }
    int32_t cases = 0;
    if (!read_all(in, &cases, sizeof cases) || cases < 0) return 3;
    for (int c = 0; c < cases; ++c) {
        int32_t head[4];
        if (!read_all(in, head, sizeof head)) return 3;
        const int degree = head[0], K = head[1], F = head[2], N = head[3];
        if (degree < 0 || degree > kMaxDegree || K < num_coeffs(degree) || F < 0 || N < 0) {
            fprintf(stderr, "case %d: degree=%d K=%d F=%d N=%d\n", c, degree, K, F, N);
            return 3;
        }
        const size_t rows = (size_t)F * N;
        std::vector<float> means(rows * 3), campos((size_t)F * 3), sh(rows * 3 * K), grad(rows * 3);
        if (!read_all(in, means.data(), means.size() * 4) || !read_all(in, campos.data(), campos.size() * 4) ||
            !read_all(in, sh.data(), sh.size() * 4) || !read_all(in, grad.data(), grad.size() * 4))
            return 3;
        std::vector<float> colors(rows * 3), grad_sh(rows * 3 * K), grad_means(rows * 3);
        auto go = [&](auto fn) {
            fn(K, F, N, means.data(), campos.data(), sh.data(), grad.data(), colors.data(), grad_sh.data(), grad_means.data());
        };
        switch (degree) {
            case 0: go(run_case<0>); break;
            case 1: go(run_case<1>); break;
            case 2: go(run_case<2>); break;
            case 3: go(run_case<3>); break;
            default: go(run_case<4>); break;
        }
        fwrite(colors.data(), 4, colors.size(), out);
        fwrite(grad_sh.data(), 4, grad_sh.size(), out);
        fwrite(grad_means.data(), 4, grad_means.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
