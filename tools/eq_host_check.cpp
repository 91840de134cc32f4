// Stand-alone check of csrc/eq.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/eq_host_check.cpp -o /tmp/eq_host_check && /tmp/eq_host_check
//
// It drives the host twin of the equaliser (eq_run_host: the scalar routines the GPU kernels share) over 8, 32, 44.1 and 192 kHz,
// 1, 3 and 6 sections, and lengths around a run of 16 samples, a span of 8192 and a chunk of two spans, zero and one sample;
// noise, a tone, silence, an impulse, a signal with a NaN and infinities --, single clips and packed batches at odd offsets over
// several designs, out of place and in place.  The samples are a heap block of exactly n_x floats, the workspace a heap block of
// exactly the bytes eq_layout states and the records a heap block of exactly n_clips records, so a read or write past any of
// them is a sanitizer report.  It also holds the twin to a plain serial fp64 cascade (half an fp32 ulp of the sample plus 2e-10 of
// the clip's peak; the figure it prints is the worst distance found beyond the half ulp), a packed clip to the same clip alone
// (the same bits), a NaN clip to its input, and every write to the inside of its clip.  Exit status 0 only when all held.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "eq.h"

using namespace gsv;

namespace {

long g_calls = 0, g_clips = 0, g_fail = 0;
double g_worst = 0.0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;
const double kPi = 3.14159265358979323846;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

std::vector<float> signal(int kind, int n, int rate) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 1: x[i] = (float)(0.5 * sin(2.0 * kPi * 60.0 * i / rate)); break;
            case 2: x[i] = 0.f; break;
            case 3: x[i] = i == 0 ? 1.f : 0.f; break;
            default: x[i] = (float)(2.0 * uniform() - 1.0); break;
        }
    }
    if (kind == 4 && n > 2) {
        x[n / 3] = std::numeric_limits<float>::quiet_NaN();
        x[n / 2] = std::numeric_limits<float>::infinity();
        x[2 * n / 3] = -std::numeric_limits<float>::infinity();
    }
    return x;
}

void fail(const char* what, int rate, int n, int kind) {
    fprintf(stderr, "rate %d n %d kind %d: %s\n", rate, n, kind, what);
    ++g_fail;
}

// cookbook sections: kind 0 high pass, 1 low pass, 2 peak, 3 low shelf, 4 high shelf
void section(int kind, double f0, double q, double gain_db, int rate, double* c) {
    const double A = pow(10.0, gain_db / 40.0), w0 = 2.0 * kPi * f0 / rate, al = sin(w0) / (2.0 * q), cs = cos(w0), r = 2.0 * sqrt(A) * al;
    double b0, b1, b2, a0, a1, a2;
    switch (kind) {
        case 0: b0 = (1 + cs) / 2; b1 = -(1 + cs); b2 = b0; a0 = 1 + al; a1 = -2 * cs; a2 = 1 - al; break;
        case 1: b0 = (1 - cs) / 2; b1 = 1 - cs; b2 = b0; a0 = 1 + al; a1 = -2 * cs; a2 = 1 - al; break;
        case 2: b0 = 1 + al * A; b1 = -2 * cs; b2 = 1 - al * A; a0 = 1 + al / A; a1 = -2 * cs; a2 = 1 - al / A; break;
        case 3:
            b0 = A * ((A + 1) - (A - 1) * cs + r); b1 = 2 * A * ((A - 1) - (A + 1) * cs); b2 = A * ((A + 1) - (A - 1) * cs - r);
            a0 = (A + 1) + (A - 1) * cs + r; a1 = -2 * ((A - 1) + (A + 1) * cs); a2 = (A + 1) + (A - 1) * cs - r;
            break;
        default:
            b0 = A * ((A + 1) + (A - 1) * cs + r); b1 = -2 * A * ((A - 1) + (A + 1) * cs); b2 = A * ((A + 1) + (A - 1) * cs - r);
            a0 = (A + 1) - (A - 1) * cs + r; a1 = 2 * ((A - 1) - (A + 1) * cs); a2 = (A + 1) - (A - 1) * cs - r;
            break;
    }
    c[0] = b0 / a0; c[1] = b1 / a0; c[2] = b2 / a0; c[3] = a1 / a0; c[4] = a2 / a0;
}

EqCoefs design(int count, int rate) {
    EqCoefs d;
    memset(&d, 0, sizeof d);
    d.n_sections = count;
    const double top = 0.45 * rate;
    if (count == 1) {
        section(2, 1000.0, 2.0, 6.0, rate, d.c[0]);
    } else if (count == 3) {        // the "voice" preset
        section(0, 80.0, 1.0 / sqrt(2.0), 0.0, rate, d.c[0]);
        section(2, 300.0, 1.0, 2.5, rate, d.c[1]);
        section(2, fmin(7000.0, top), 2.0, -3.0, rate, d.c[2]);
    } else {
        section(0, 20.0, 0.5, 0.0, rate, d.c[0]);
        section(3, 120.0, 0.7, 4.0, rate, d.c[1]);
        section(2, 300.0, 1.0, 2.5, rate, d.c[2]);
        section(2, fmin(2500.0, 0.3 * rate), 4.0, -6.0, rate, d.c[3]);
        section(4, fmin(6000.0, 0.4 * rate), 0.8, 3.0, rate, d.c[4]);
        section(1, top, 1.0 / sqrt(2.0), 0.0, rate, d.c[5]);
    }
    return d;
}

// the definition: section after section, plain and serial
std::vector<double> serial(const std::vector<float>& x, const EqCoefs& d) {
    std::vector<double> y(x.begin(), x.end());
    for (int s = 0; s < d.n_sections; ++s) {
        const double* c = d.c[s];
        double z0 = 0, z1 = 0;
        for (double& v : y) {
            const double xn = v, yn = c[0] * xn + z0;
            z0 = c[1] * xn - c[3] * yn + z1;
            z1 = c[2] * xn - c[4] * yn;
            v = yn;
        }
    }
    return y;
}

struct Packed {
    std::unique_ptr<float[]> x, out;
    std::unique_ptr<EqRecord[]> rec;
    size_t n_x;
};

// one call through heap blocks of exactly the stated sizes; mode 0: out of place, 1: in place
Packed run(const std::vector<std::vector<float>>& clips, const std::vector<int>& index, const std::vector<EqCoefs>& designs, int gap, int mode) {
    const int B = (int)clips.size();
    std::vector<EqClip> cl((size_t)B);
    size_t at = (size_t)gap;
    for (int c = 0; c < B; ++c) {
        cl[c].offset = (long long)at; cl[c].n = (int)clips[c].size(); cl[c].design = index[c];
        at += clips[c].size() + (size_t)gap;
    }
    Packed P;
    P.n_x = at;
    P.x.reset(new float[at]);
    for (size_t i = 0; i < at; ++i) P.x[i] = -7.25f;
    for (int c = 0; c < B; ++c)
        if (!clips[c].empty()) memcpy(P.x.get() + cl[c].offset, clips[c].data(), clips[c].size() * sizeof(float));
    EqLayout L;
    if (!eq_layout(cl.data(), B, (int)designs.size(), at, true, &L, nullptr)) { ++g_fail; return P; }
    for (const EqCoefs& d : designs)
        if (!eq_coefs_ok(d)) { ++g_fail; return P; }
    std::unique_ptr<unsigned char[]> work(new unsigned char[L.bytes]);
    P.rec.reset(new EqRecord[(size_t)B]);
    float* out = P.x.get();
    if (mode == 0) {
        P.out.reset(new float[at]);
        for (size_t i = 0; i < at; ++i) P.out[i] = -14.5f;
        out = P.out.get();
    }
    eq_run_host(P.x.get(), cl.data(), B, designs.data(), (int)designs.size(), out, P.rec.get(), work.get());
    ++g_calls;
    g_clips += B;
    std::vector<char> inside(at, 0);
    for (int c = 0; c < B; ++c)
        for (int i = 0; i < cl[c].n; ++i) inside[(size_t)cl[c].offset + i] = 1;
    for (size_t i = 0; i < at; ++i) {
        if (inside[i]) continue;
        if (P.x[i] != -7.25f || (P.out && P.out[i] != -14.5f)) { fail("a write outside the clips", 0, (int)i, mode); break; }
    }
    return P;
}

void check_single(int rate, int count, int n, int kind) {
    const std::vector<float> x = signal(kind, n, rate);
    const EqCoefs d = design(count, rate);
    const Packed a = run({x}, {0}, {d}, 0, 0);
    const Packed b = run({x}, {0}, {d}, 3, 1);
    const Packed m = run({x}, {-1}, {d}, 1, 0);
    if (!a.rec || !b.rec || !m.rec) return;
    const EqRecord& r = a.rec[0];
    if (memcmp(&r, &b.rec[0], sizeof r)) fail("in place and out of place records differ", rate, n, kind);
    if (n && memcmp(a.out.get(), b.x.get() + 3, (size_t)n * sizeof(float))) fail("in place and out of place samples differ", rate, n, kind);
    if (m.rec[0].flags != (kind == 4 && n > 2 ? EQ_NONFINITE : 0) || m.rec[0].sections != 0 || memcmp(&m.rec[0].peak_in, &r.peak_in, 4) ||
        (n && memcmp(m.out.get() + 1, x.data(), (size_t)n * sizeof(float))))
        fail("measure only: record or samples", rate, n, kind);
    if (kind == 4 && n > 2) {
        if (r.flags != EQ_NONFINITE || r.sections != 0 || memcmp(a.out.get(), x.data(), (size_t)n * sizeof(float)))
            fail("a clip with a NaN did not come back as it was", rate, n, kind);
        return;
    }
    if (r.flags != EQ_EQUALISED || r.sections != count) fail("flags or section count", rate, n, kind);
    const std::vector<double> want = serial(x, d);
    double peak = 0, pin = 0, pout = 0;
    for (int i = 0; i < n; ++i) {
        peak = fmax(peak, fabs(want[i]));
        pin = fmax(pin, fabs((double)x[i]));
        pout = fmax(pout, fabs((double)a.out[i]));
    }
    if ((double)r.peak_in != pin || (double)r.peak_out != pout) fail("peaks of the record", rate, n, kind);
    for (int i = 0; i < n; ++i) {
        const double e = fabs((double)a.out[i] - want[i]), half = ldexp(fmax(fabs(want[i]), 1.1754943508222875e-38), -24);
        if (peak > 0 && (e - half) / peak > g_worst) g_worst = (e - half) / peak;
        if (e > half + 2e-10 * peak) { fail("further from the serial cascade than the fp32 rounding and 2e-10 of the peak", rate, n, kind); break; }
    }
}

void check_packed(int rate, const std::vector<int>& lengths) {
    std::vector<std::vector<float>> clips;
    std::vector<int> index;
    const std::vector<EqCoefs> designs = {design(1, rate), design(3, rate), design(6, rate)};
    int k = 0;
    for (int n : lengths) {
        clips.push_back(signal(k % 5, n, rate));
        index.push_back(k % 4 - 1);
        ++k;
    }
    const Packed all = run(clips, index, designs, 5, 0);
    if (!all.rec) return;
    size_t at = 5;
    for (size_t c = 0; c < clips.size(); ++c) {
        const Packed one = run({clips[c]}, {index[c] < 0 ? -1 : 0}, {designs[index[c] < 0 ? 0 : index[c]]}, 0, 0);
        if (!one.rec) return;
        if (memcmp(&one.rec[0], &all.rec[c], sizeof(EqRecord))) fail("a packed clip's record differs from the clip alone", rate, (int)clips[c].size(), (int)c);
        if (!clips[c].empty() && memcmp(one.out.get(), all.out.get() + at, clips[c].size() * sizeof(float)))
            fail("a packed clip's samples differ from the clip alone", rate, (int)clips[c].size(), (int)c);
        at += clips[c].size() + 5;
    }
}

}  // namespace

int main() {
    static const int kRates[] = {8000, 32000, 44100, 192000};
    static const int kCounts[] = {1, 3, 6};
    const auto t0 = std::chrono::steady_clock::now();
    for (int rate : kRates) {
        const std::vector<int> lengths = {0, 1, EQ_R - 1, EQ_R, EQ_R + 1, EQ_SPAN - 1, EQ_SPAN, EQ_SPAN + 1, EQ_CHUNK - 1, EQ_CHUNK, EQ_CHUNK + 1,
                                          3 * EQ_CHUNK + 5};
        for (int count : kCounts)
            for (int n : lengths)
                for (int kind = 0; kind < 5; ++kind) check_single(rate, count, n, kind);
        check_packed(rate, {777, 0, 3 * EQ_SPAN, EQ_R, 2 * EQ_CHUNK + 1, 1, EQ_CHUNK + 1, 2 * EQ_CHUNK, 5 * EQ_CHUNK + 3});
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%ld calls, %ld clips, %ld failed expectations, worst distance beyond the rounding %.3g of the peak, %.2f s\n", g_calls, g_clips,
           g_fail, g_worst, s);
    return g_fail || !g_calls ? 1 : 0;
}
