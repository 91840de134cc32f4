// Stand-alone check of csrc/reverb.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/reverb_host_check.cpp -o /tmp/reverb_host_check && /tmp/reverb_host_check
//
// It drives the host twin of the reverb (rvb_run_host: the scalar routines the GPU kernels share) over the "tiny" parameter set of
// the tests -- combs of 1, 2, 3, 5, 7, 64, 65 and 257 samples, all-passes of 1, 3, 63 and 130: degenerate lines and lines that are
// no multiple of a lane's run, dozens of wraps in a short clip --, a set with lines longer than a span (2049 and 4100 samples: read
// back from the plane, a short last span) and the "voice" set at 8 kHz, at every length around the shortest and the longest delay up
// to three wraps plus 7; noise, an impulse, a gated tone, a clip of 1e-30 amplitude, a signal with a NaN and infinities; single clips
// and packed batches at odd offsets with guard words before, between and behind, over several sets and -1, out of place and in
// place.  The samples are a heap block of exactly n_x floats, the workspace a heap block of exactly the bytes rvb_layout states and
// the records a heap block of exactly n_clips records, so a read or write past any of them is a sanitizer report.  It also holds the
// twin to a plain serial fp64 loop (one fp32 ulp of the sample plus 1e-12 of the largest reachable level), a packed clip to the same
// clip alone (the same bits), a NaN clip to its input, and every write to the inside of its clip.  Exit status 0 only when all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "reverb.h"

using namespace gsv;

namespace {

long g_calls = 0, g_clips = 0, g_fail = 0, g_differ = 0, g_samples = 0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;
const double kPi = 3.14159265358979323846;
const float kFill = -7.25f;
const int kGuard = 5;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

RvbParams make(const int (&comb)[8], const int (&ap)[4], double room, double damping, double wet, double dry) {
    RvbParams p;
    memcpy(p.comb, comb, sizeof p.comb);
    memcpy(p.allpass, ap, sizeof p.allpass);
    p.d = 0.4 * damping;
    p.fb = 0.28 * room + 0.7;
    p.gin = 0.015;
    p.gw = 1.5 * wet * 2.0;
    p.gd = 2.0 * dry;
    return p;
}

std::vector<RvbParams> sets() {
    const int tc[8] = {1, 2, 3, 5, 7, 64, 65, 257}, ta[4] = {1, 3, 63, 130};
    const int lc[8] = {2049, 4100, 300, 31, 33, 2048, 2047, 1000}, la[4] = {2500, 17, 256, 255};
    int vc[8], va[4];
    const int tun_c[8] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617}, tun_a[4] = {556, 441, 341, 225};
    for (int k = 0; k < 8; ++k) vc[k] = 8000 * tun_c[k] / 44100;
    for (int j = 0; j < 4; ++j) va[j] = 8000 * tun_a[j] / 44100;
    return {make(tc, ta, 0.1, 0.5, 0.03, 0.97), make(lc, la, 1.0, 0.0, 1.0, 0.0), make(vc, va, 0.1, 0.5, 0.03, 0.97)};
}

// kind 0 noise, 1 impulse, 2 gated 220 Hz tone, 3 noise of 1e-30 amplitude, 4 noise with a NaN and infinities
std::vector<float> signal(int kind, int n) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 1: x[i] = i == 0 ? 1.f : 0.f; break;
            case 2: x[i] = (float)(((i / 400) % 2 ? 0.0 : 0.8) * sin(2.0 * kPi * 220.0 * i / 32000.0)); break;
            case 3: x[i] = (float)(1e-30 * (2.0 * uniform() - 1.0)); break;
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

// the definition, one sample after the other
std::vector<float> serial(const std::vector<float>& x, const RvbParams& p) {
    std::vector<std::vector<double>> bk(8), ak(4);
    for (int k = 0; k < 8; ++k) bk[k].assign((size_t)p.comb[k], 0.0);
    for (int j = 0; j < 4; ++j) ak[j].assign((size_t)p.allpass[j], 0.0);
    double lk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<float> y(x.size());
    for (size_t i = 0; i < x.size(); ++i) {
        const double v = x[i];
        volatile double u = p.gin * v;
        double s = 0.0;
        for (int k = 0; k < 8; ++k) {
            double& slot = bk[k][i % (size_t)p.comb[k]];
            const double o = slot;
            volatile double a = o * (1.0 - p.d), b = lk[k] * p.d;
            lk[k] = a + b;
            volatile double c = lk[k] * p.fb;
            slot = u + c;
            s = k == 0 ? o : s + o;
        }
        for (int j = 0; j < 4; ++j) {
            double& slot = ak[j][i % (size_t)p.allpass[j]];
            const double t = slot;
            slot = s + 0.5 * t;
            s = t - s;
        }
        volatile double w1 = s * p.gw, w2 = v * p.gd;
        y[i] = loud_store(w1 + w2);
    }
    return y;
}

double gain_bound(const RvbParams& p) { return fabs(p.gd) + fabs(p.gw) * 8.0 * fabs(p.gin) / (1.0 - p.fb) * 81.0; }

void fail(const char* what, long a = 0, long b = 0) {
    if (++g_fail <= 20) fprintf(stderr, "FAIL %s (%ld, %ld)\n", what, a, b);
}

struct Result {
    std::vector<float> out;
    std::vector<RvbRecord> recs;
};

// one call over exact heap blocks; clips packed between guard words
Result run(const std::vector<std::vector<float>>& clips, const std::vector<int>& index, const std::vector<RvbParams>& params, bool inplace) {
    size_t n_x = (size_t)kGuard;
    for (const auto& c : clips) n_x += c.size() + (size_t)kGuard;
    std::unique_ptr<float[]> x(new float[n_x]), out(new float[n_x]);
    std::vector<RvbClip> tab(clips.size());
    size_t at = (size_t)kGuard;
    for (size_t i = 0; i < n_x; ++i) { x[i] = kFill; out[i] = 2 * kFill; }
    for (size_t c = 0; c < clips.size(); ++c) {
        if (!clips[c].empty()) memcpy(&x[at], clips[c].data(), clips[c].size() * sizeof(float));
        tab[c].offset = (long long)at;
        tab[c].n = (int32_t)clips[c].size();
        tab[c].design = index[c];
        at += clips[c].size() + (size_t)kGuard;
    }
    RvbLayout L;
    if (!rvb_layout(tab.data(), (int)tab.size(), (int)params.size(), n_x, true, &L, nullptr)) {
        fail("layout");
        return {};
    }
    std::unique_ptr<unsigned char[]> work(new unsigned char[L.bytes]);
    memset(work.get(), 0xA5, L.bytes);
    std::unique_ptr<RvbRecord[]> recs(new RvbRecord[tab.size()]);
    float* dst = inplace ? x.get() : out.get();
    rvb_run_host(x.get(), tab.data(), (int)tab.size(), params.data(), (int)params.size(), dst, recs.get(), work.get());
    ++g_calls;
    g_clips += (long)tab.size();
    // nothing outside a clip moved
    std::vector<char> inside(n_x, 0);
    for (const auto& t : tab)
        for (int i = 0; i < t.n; ++i) inside[(size_t)t.offset + (size_t)i] = 1;
    for (size_t i = 0; i < n_x; ++i)
        if (!inside[i] && dst[i] != (inplace ? kFill : 2 * kFill)) fail("write outside a clip", (long)i);
    Result r;
    r.out.assign(dst, dst + n_x);
    r.recs.assign(recs.get(), recs.get() + tab.size());
    return r;
}

bool finite_clip(const std::vector<float>& x) {
    for (float v : x)
        if (!std::isfinite(v)) return false;
    return true;
}

void check_against_serial(const float* got, const std::vector<float>& x, const RvbParams& p, long tag) {
    const std::vector<float> want = serial(x, p);
    double peak = 0.0;
    for (float v : x) peak = fmax(peak, fabs((double)v));
    const double slack = 1e-12 * fmax(1.0, peak * gain_bound(p));
    for (size_t i = 0; i < x.size(); ++i) {
        ++g_samples;
        if (memcmp(&got[i], &want[i], 4) != 0) ++g_differ;
        const double a = fabs((double)want[i]);
        const double ulp = (double)nextafterf((float)a, INFINITY) - a;
        if (!(fabs((double)got[i] - (double)want[i]) <= ulp + slack)) fail("twin against the serial loop", tag, (long)i);
    }
}

std::vector<int> lengths(const RvbParams& p) {
    int lo = p.comb[0], hi = p.comb[0];
    for (int k = 0; k < 8; ++k) { lo = p.comb[k] < lo ? p.comb[k] : lo; hi = p.comb[k] > hi ? p.comb[k] : hi; }
    for (int j = 0; j < 4; ++j) { lo = p.allpass[j] < lo ? p.allpass[j] : lo; hi = p.allpass[j] > hi ? p.allpass[j] : hi; }
    return {0, 1, lo - 1 > 0 ? lo - 1 : 0, lo, lo + 1, hi - 1, hi, hi + 1, 2 * hi + 1, 3 * hi + 7};
}

}  // namespace

int main() {
    const std::vector<RvbParams> P = sets();
    for (size_t s = 0; s < P.size(); ++s) {
        if (rvb_params_bad(P[s])) fail("a set of the check is refused", (long)s);
        // every length with every signal, each clip alone and all of a set packed
        std::vector<std::vector<float>> all;
        for (int n : lengths(P[s]))
            for (int kind = 0; kind < 5; ++kind) all.push_back(signal(kind, n));
        const std::vector<int> idx(all.size(), 0);
        for (int inplace = 0; inplace < 2; ++inplace) {
            const Result packed = run(all, idx, {P[s]}, inplace != 0);
            if (packed.recs.size() != all.size()) continue;
            size_t at = (size_t)kGuard;
            for (size_t c = 0; c < all.size(); ++c) {
                const std::vector<float>& x = all[c];
                const float* got = packed.out.data() + at;
                const RvbRecord& r = packed.recs[c];
                if (finite_clip(x)) {
                    if (r.flags != RVB_REVERBED) fail("flags of a finite clip", (long)s, (long)c);
                    if (!inplace) check_against_serial(got, x, P[s], (long)(s * 1000 + c));
                    const Result alone = run({x}, {0}, {P[s]}, false);
                    if (!x.empty() && memcmp(alone.out.data() + kGuard, got, x.size() * 4) != 0) fail("packed against alone", (long)s, (long)c);
                    if (memcmp(&alone.recs[0], &r, sizeof r) != 0) fail("record packed against alone", (long)s, (long)c);
                } else {
                    if (r.flags != RVB_NONFINITE) fail("flags of a non-finite clip", (long)s, (long)c);
                    if (memcmp(got, x.data(), x.size() * 4) != 0) fail("a non-finite clip moved", (long)s, (long)c);
                    if (memcmp(&r.peak_in, &r.peak_out, 4) != 0) fail("peaks of a non-finite clip", (long)s, (long)c);
                }
                at += x.size() + (size_t)kGuard;
            }
        }
    }
    // a mixed batch over all the sets and -1
    {
        std::vector<std::vector<float>> clips = {signal(0, 5001), signal(2, 777), {}, signal(4, 4000), signal(0, 9000), signal(1, 1), signal(0, 8300)};
        const std::vector<int> idx = {0, 1, 2, 2, -1, 1, 1};
        for (int inplace = 0; inplace < 2; ++inplace) {
            const Result r = run(clips, idx, P, inplace != 0);
            if (r.recs.size() != clips.size()) continue;
            size_t at = (size_t)kGuard;
            for (size_t c = 0; c < clips.size(); ++c) {
                const float* got = r.out.data() + at;
                if (idx[c] < 0 || !finite_clip(clips[c])) {
                    if (memcmp(got, clips[c].data(), clips[c].size() * 4) != 0) fail("a copied clip moved", (long)c);
                    if (r.recs[c].flags != (idx[c] < 0 ? 0 : RVB_NONFINITE)) fail("flags of a copied clip", (long)c);
                } else if (!inplace) {
                    check_against_serial(got, clips[c], P[(size_t)idx[c]], 9000 + (long)c);
                }
                at += clips[c].size() + (size_t)kGuard;
            }
            const Result none = run(clips, std::vector<int>(clips.size(), -1), {}, inplace != 0);
            (void)none;
        }
    }
    printf("reverb_host_check: %ld calls, %ld clips, %ld samples against the serial loop (%ld differ in a bit), %ld failures\n", g_calls, g_clips,
           g_samples, g_differ, g_fail);
    return g_fail ? 1 : 0;
}
