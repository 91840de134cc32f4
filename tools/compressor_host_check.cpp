// Stand-alone check of csrc/compressor.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/compressor_host_check.cpp -o /tmp/compressor_host_check && /tmp/compressor_host_check
//
// It drives the host twin of the compressor (cmp_run_host: the scalar routines the GPU kernels share) over 8, 32 and 48 kHz, four
// parameter sets -- "voice", a fast one, a slow one with makeup, ratio inf -- and lengths around a run of 16 samples, a span of 8192
// and a chunk of two spans, zero and one sample; noise, a gated tone, a full-scale square, a clip under the threshold, a signal
// with a NaN and infinities --, single clips and packed batches at odd offsets over several sets, out of place and in place.  The
// samples are a heap block of exactly n_x floats, the workspace a heap block of exactly the bytes cmp_layout states and the records
// a heap block of exactly n_clips records, so a read or write past any of them is a sanitizer report.  It also holds the twin to a
// plain serial fp64 loop with libm's log2 and exp2 (one fp32 ulp of the sample), a packed clip to the same clip alone (the same
// bits), a NaN clip and a clip under its threshold to their input, and every write to the inside of its clip.  Exit status 0 only
// when all held.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "compressor.h"

using namespace gsv;

namespace {

long g_calls = 0, g_clips = 0, g_fail = 0, g_differ = 0, g_samples = 0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;
const double kPi = 3.14159265358979323846;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

// threshold_db, ratio, attack_ms, release_ms, makeup_db
const double kSets[4][5] = {{-18.0, 3.5, 1.0, 100.0, 0.0}, {-30.0, 20.0, 0.1, 5.0, 0.0}, {-6.0, 2.0, 30.0, 1000.0, 3.0},
                            {-18.0, INFINITY, 1.0, 100.0, 0.0}};

CmpParams params(int set, int rate) {
    const double* p = kSets[set];
    CmpParams d;
    d.attack = exp(-2.0 * kPi * 1000.0 / (rate * p[2]));
    d.release = exp(-2.0 * kPi * 1000.0 / (rate * p[3]));
    d.threshold = pow(10.0, p[0] / 20.0);
    d.slope = 1.0 / p[1] - 1.0;
    d.makeup = pow(10.0, p[4] / 20.0);
    return d;
}

// kind 0 noise, 1 gated 220 Hz tone, 2 full-scale square, 3 noise 26 dB under the set's threshold, 4 noise with a NaN and infinities
std::vector<float> signal(int kind, int n, int rate, int set) {
    std::vector<float> x((size_t)n);
    const double quiet = pow(10.0, (kSets[set][0] - 26.0) / 20.0);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 1: x[i] = (float)(((i / 3001) % 2 ? 0.01 : 0.9) * sin(2.0 * kPi * 220.0 * i / rate)); break;
            case 2: x[i] = (i / 32) % 2 ? -1.f : 1.f; break;
            case 3: x[i] = (float)(quiet * (2.0 * uniform() - 1.0)); break;
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

// the definition, plain and serial, libm's log2 and exp2
std::vector<float> serial(const std::vector<float>& x, const CmpParams& d, double* min_gain) {
    std::vector<float> y(x.size());
    double p = 0, e = 0, gm = 1.0;
    const double inv = 1.0 / d.threshold;
    for (size_t i = 0; i < x.size(); ++i) {
        const double ax = fabs((double)x[i]), t = d.release * p + (1.0 - d.release) * ax;
        p = t > ax ? t : ax;
        e = d.attack * e + (1.0 - d.attack) * p;
        const double g = e <= d.threshold ? 1.0 : exp2(d.slope * log2(e * inv));
        gm = fmin(gm, g);
        y[i] = (float)fmin(fmax(d.makeup * g * (double)x[i], -3.4028234663852886e38), 3.4028234663852886e38);
    }
    *min_gain = gm;
    return y;
}

long ulps(float a, float b) {
    int32_t i, j;
    memcpy(&i, &a, 4);
    memcpy(&j, &b, 4);
    const long u = i < 0 ? -(long)(i & 0x7FFFFFFF) : i, v = j < 0 ? -(long)(j & 0x7FFFFFFF) : j;
    return labs(u - v);
}

struct Packed {
    std::unique_ptr<float[]> x, out;
    std::unique_ptr<CmpRecord[]> rec;
    size_t n_x;
};

// one call through heap blocks of exactly the stated sizes; mode 0: out of place, 1: in place
Packed run(const std::vector<std::vector<float>>& clips, const std::vector<int>& index, const std::vector<CmpParams>& sets, int gap, int mode) {
    const int B = (int)clips.size();
    std::vector<CmpClip> cl((size_t)B);
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
    CmpLayout L;
    if (!cmp_layout(cl.data(), B, (int)sets.size(), at, true, &L, nullptr)) { ++g_fail; return P; }
    for (const CmpParams& d : sets)
        if (!cmp_params_ok(d)) { ++g_fail; return P; }
    std::unique_ptr<unsigned char[]> work(new unsigned char[L.bytes]);
    P.rec.reset(new CmpRecord[(size_t)B]);
    float* out = P.x.get();
    if (mode == 0) {
        P.out.reset(new float[at]);
        for (size_t i = 0; i < at; ++i) P.out[i] = -14.5f;
        out = P.out.get();
    }
    cmp_run_host(P.x.get(), cl.data(), B, sets.data(), (int)sets.size(), out, P.rec.get(), work.get());
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

void check_single(int rate, int set, int n, int kind) {
    const std::vector<float> x = signal(kind, n, rate, set);
    const CmpParams d = params(set, rate);
    const Packed a = run({x}, {0}, {d}, 0, 0);
    const Packed b = run({x}, {0}, {d}, 3, 1);
    const Packed m = run({x}, {-1}, {d}, 1, 0);
    if (!a.rec || !b.rec || !m.rec) return;
    const CmpRecord& r = a.rec[0];
    if (memcmp(&r, &b.rec[0], sizeof r)) fail("in place and out of place records differ", rate, n, kind);
    if (n && memcmp(a.out.get(), b.x.get() + 3, (size_t)n * sizeof(float))) fail("in place and out of place samples differ", rate, n, kind);
    if (m.rec[0].flags != (kind == 4 && n > 2 ? CMP_NONFINITE : 0) || m.rec[0].min_gain != 1.f || memcmp(&m.rec[0].peak_in, &r.peak_in, 4) ||
        (n && memcmp(m.out.get() + 1, x.data(), (size_t)n * sizeof(float))))
        fail("measure only: record or samples", rate, n, kind);
    if (kind == 4 && n > 2) {
        if (r.flags != CMP_NONFINITE || r.min_gain != 1.f || memcmp(a.out.get(), x.data(), (size_t)n * sizeof(float)))
            fail("a clip with a NaN did not come back as it was", rate, n, kind);
        return;
    }
    double gm = 1.0;
    const std::vector<float> want = serial(x, d, &gm);
    double pin = 0, pout = 0;
    for (int i = 0; i < n; ++i) {
        pin = fmax(pin, fabs((double)x[i]));
        pout = fmax(pout, fabs((double)a.out[i]));
        const long u = ulps(a.out[i], want[i]);
        g_differ += u != 0;
        if (u > 1) { fail("more than one fp32 ulp from the serial definition", rate, n, kind); break; }
    }
    g_samples += n;
    if ((double)r.peak_in != pin || (double)r.peak_out != pout) fail("peaks of the record", rate, n, kind);
    if (fabs((double)r.min_gain / gm - 1.0) > 1.2e-7 || r.flags != (r.min_gain < 1.f ? CMP_COMPRESSED : 0)) fail("min_gain or flags", rate, n, kind);
    if (kind == 3 && (r.flags != 0 || (d.makeup == 1.0 && n && memcmp(a.out.get(), x.data(), (size_t)n * sizeof(float)))))
        fail("a clip under its threshold did not come back as it was", rate, n, kind);
}

void check_packed(int rate, const std::vector<int>& lengths) {
    std::vector<std::vector<float>> clips;
    std::vector<int> index;
    const std::vector<CmpParams> sets = {params(0, rate), params(1, rate), params(2, rate)};
    int k = 0;
    for (int n : lengths) {
        clips.push_back(signal(k % 5, n, rate, 0));
        index.push_back(k % 4 - 1);
        ++k;
    }
    const Packed all = run(clips, index, sets, 5, 0);
    if (!all.rec) return;
    size_t at = 5;
    for (size_t c = 0; c < clips.size(); ++c) {
        const Packed one = run({clips[c]}, {index[c] < 0 ? -1 : 0}, {sets[index[c] < 0 ? 0 : index[c]]}, 0, 0);
        if (!one.rec) return;
        if (memcmp(&one.rec[0], &all.rec[c], sizeof(CmpRecord))) fail("a packed clip's record differs from the clip alone", rate, (int)clips[c].size(), (int)c);
        if (!clips[c].empty() && memcmp(one.out.get(), all.out.get() + at, clips[c].size() * sizeof(float)))
            fail("a packed clip's samples differ from the clip alone", rate, (int)clips[c].size(), (int)c);
        at += clips[c].size() + 5;
    }
}

}  // namespace

int main() {
    static const int kRates[] = {8000, 32000, 48000};
    const auto t0 = std::chrono::steady_clock::now();
    for (int rate : kRates) {
        const std::vector<int> lengths = {0, 1, CMP_R - 1, CMP_R, CMP_R + 1, CMP_SPAN - 1, CMP_SPAN, CMP_SPAN + 1, CMP_CHUNK - 1, CMP_CHUNK,
                                          CMP_CHUNK + 1, 3 * CMP_CHUNK + 5};
        for (int set = 0; set < 4; ++set)
            for (int n : lengths)
                for (int kind = 0; kind < 5; ++kind) check_single(rate, set, n, kind);
        check_packed(rate, {777, 0, 3 * CMP_SPAN, CMP_R, 2 * CMP_CHUNK + 1, 1, CMP_CHUNK + 1, 2 * CMP_CHUNK, 5 * CMP_CHUNK + 3});
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%ld calls, %ld clips, %ld failed expectations, %ld of %ld samples one ulp from the serial definition, %.2f s\n", g_calls, g_clips,
           g_fail, g_differ, g_samples, s);
    return g_fail || !g_calls ? 1 : 0;
}
