// Stand-alone check of csrc/limiter.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/limiter_host_check.cpp -o /tmp/limiter_host_check && /tmp/limiter_host_check
//
// It drives the host twin of the true-peak limiter (lim_run_host: the scalar routines the GPU kernels share) over the edge lengths
// of the tests -- 0, 1, around the 12 taps, around the look-ahead, around the scan tile and into a third tile -- with a sine above
// the ceiling, clicks at both ends and on a tile edge, noise, silence and a NaN; look-aheads of 1, 48 and the longest the ABI takes;
// single clips and one packed batch at odd offsets; out of place, in place and measure only.  The samples are a heap block of
// exactly n_x floats, the workspace a heap block of exactly the bytes lim_layout states and the records a heap block of exactly
// n_clips records, so a read or write past any of them is a sanitizer report.  It also holds 0 < g <= c, r <= h <= c, |y| <= |x|, an
// untouched clip to its bits, a packed clip to the same clip alone, and every write to the inside of its clip.  Exit status 0 only
// when all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "limiter.h"

using namespace gsv;

namespace {

long g_calls = 0, g_fail = 0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

void expect(bool ok, const char* what, int n, int kind, int look) {
    if (ok) return;
    ++g_fail;
    std::fprintf(stderr, "FAILED: %s (n %d, signal %d, look-ahead %d)\n", what, n, kind, look);
}

std::vector<float> signal(int kind, int n) {
    std::vector<float> x((size_t)n, 0.f);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 0: x[i] = (float)(1.2 * std::sin(2.0 * 3.14159265358979323846 * 997.0 * i / 32000.0)); break;
            case 1: x[i] = (float)(2.4 * uniform() - 1.2); break;
            case 4: x[i] = (float)(0.3 * std::sin(0.2 * i)); break;
            case 5: x[i] = (float)(uniform() - 0.5); break;
            default: break;
        }
    }
    if (n) {
        if (kind == 2) x[0] = 1.5f, x[(size_t)n - 1] = -1.5f;
        if (kind == 3) x[n > LIM_TILE ? LIM_TILE : n / 2] = 1.5f;
        if (kind == 5) x[(size_t)n / 3] = NAN;
    }
    return x;
}

struct Result { std::vector<float> y; std::vector<LimRecord> rec; };

// one call over heap blocks of exactly the stated sizes; mode 0 measure only, 1 out of place, 2 in place
Result run(const std::vector<float>& packed, const std::vector<LimClip>& clips, int look, int rel, int mode, std::vector<unsigned char>* keep) {
    const size_t n_x = packed.size();
    std::unique_ptr<float[]> x(new float[n_x]), out(new float[n_x]);
    if (n_x) std::memcpy(x.get(), packed.data(), n_x * sizeof(float));
    for (size_t i = 0; i < n_x; ++i) out[i] = -7.25f;
    LimLayout L;
    if (!lim_layout(clips.data(), (int)clips.size(), n_x, true, &L, nullptr)) { ++g_fail; return {}; }
    std::unique_ptr<unsigned char[]> work(new unsigned char[L.bytes]);
    std::unique_ptr<LimRecord[]> rec(new LimRecord[clips.size()]);
    float* o = mode == 0 ? nullptr : mode == 1 ? out.get() : x.get();
    lim_run_host(x.get(), clips.data(), (int)clips.size(), look, rel, o, rec.get(), work.get());
    ++g_calls;
    Result r;
    r.y.assign(mode == 1 ? out.get() : x.get(), (mode == 1 ? out.get() : x.get()) + n_x);
    r.rec.assign(rec.get(), rec.get() + clips.size());
    if (keep) keep->assign(work.get(), work.get() + L.bytes);
    return r;
}

void check_single(int kind, int n, int look, int rel) {
    const std::vector<float> x = signal(kind, n);
    const std::vector<LimClip> clip = {{0, n, -1.f}};
    std::vector<unsigned char> work;
    const Result a = run(x, clip, look, rel, 1, &work), b = run(x, clip, look, rel, 2, nullptr), m = run(x, clip, look, rel, 0, nullptr);
    if (a.rec.empty() || b.rec.empty() || m.rec.empty()) return;
    const LimRecord& r = a.rec[0];
    expect(std::memcmp(&a.rec[0], &b.rec[0], sizeof(LimRecord)) == 0 && (n == 0 || std::memcmp(a.y.data(), b.y.data(), (size_t)n * 4) == 0),
           "in place differs from out of place", n, kind, look);
    expect((n == 0 || std::memcmp(m.y.data(), x.data(), (size_t)n * 4) == 0) && std::memcmp(&m.rec[0].true_peak_in, &r.true_peak_in, 4) == 0 &&
               !(m.rec[0].flags & LIM_LIMITED),
           "measure only", n, kind, look);
    const bool limited = r.flags & LIM_LIMITED;
    if (!limited) expect(n == 0 || std::memcmp(a.y.data(), x.data(), (size_t)n * 4) == 0, "an untouched clip moved", n, kind, look);
    expect(((r.flags & LIM_NONFINITE) != 0) == (kind == 5 && n > 0), "nonfinite flag", n, kind, look);
    expect(kind != 4 || !limited, "a clip under the ceiling was limited", n, kind, look);
    expect(kind != 2 || n == 0 || limited, "a click was not limited", n, kind, look);
    if (r.flags & LIM_NONFINITE) return;
    LimLayout L;
    lim_layout(clip.data(), 1, (size_t)n, true, &L, nullptr);
    auto arr = [&](size_t off) { return reinterpret_cast<const float*>(work.data() + off); };
    const float *c = arr(L.c_off), *h = arr(L.h_off), *rr = arr(L.r_off), *g = arr(L.g_off);
    const float T = (float)std::pow(10.0, -1.0 / 20.0);
    float gmin = 1.f;
    bool ok = true;
    for (int i = 0; i < n; ++i) {
        ok = ok && c[i] > 0.f && c[i] <= 1.f && h[i] <= c[i] && rr[i] <= h[i] && rr[i] > 0.f && g[i] > 0.f && g[i] <= c[i];
        ok = ok && std::fabs(a.y[i]) <= std::fabs(x[i]) && (x[i] == 0.f || a.y[i] != 0.f);
        gmin = g[i] < gmin ? g[i] : gmin;
    }
    expect(ok, "stage order 0 < g <= c, r <= h <= c, |y| <= |x|", n, kind, look);
    expect(limited == (r.true_peak_in > T) && limited == (r.min_gain < 1.f) && r.min_gain == gmin, "record consistency", n, kind, look);
    expect(!limited || r.true_peak_out <= T * (1.f + 2.4e-7f), "true peak out above the ceiling", n, kind, look);
}

void check_packed(int look, int rel) {
    const int lens[] = {LIM_TILE + 1, 97, 2 * LIM_TILE + 47, 0, 49, LIM_TILE - 1, 13};
    const int kinds[] = {2, 4, 1, 0, 5, 0, 1};
    const float ceil_db[] = {-1.f, -1.f, -3.f, -1.f, -1.f, NAN, -6.f};
    const int guard = 5;
    std::vector<float> packed((size_t)guard, -7.25f);
    std::vector<LimClip> clips;
    std::vector<std::vector<float>> xs;
    for (int k = 0; k < 7; ++k) {
        xs.push_back(signal(kinds[k], lens[k]));
        clips.push_back({(long long)packed.size(), lens[k], ceil_db[k]});
        packed.insert(packed.end(), xs.back().begin(), xs.back().end());
        packed.insert(packed.end(), (size_t)guard, -7.25f);
    }
    const Result p = run(packed, clips, look, rel, 1, nullptr);
    if (p.rec.empty()) return;
    std::vector<bool> inside(packed.size(), false);
    for (int k = 0; k < 7; ++k) {
        const Result s = run(xs[k], {{0, lens[k], ceil_db[k]}}, look, rel, 1, nullptr);
        expect(std::memcmp(&s.rec[0], &p.rec[k], sizeof(LimRecord)) == 0 &&
                   (lens[k] == 0 || std::memcmp(s.y.data(), p.y.data() + clips[k].offset, (size_t)lens[k] * 4) == 0),
               "a packed clip differs from the clip alone", lens[k], kinds[k], look);
        for (int i = 0; i < lens[k]; ++i) inside[(size_t)clips[k].offset + i] = true;
    }
    bool ok = true;
    for (size_t i = 0; i < packed.size(); ++i) ok = ok && (inside[i] || p.y[i] == -7.25f);
    expect(ok, "written outside a clip", 0, -1, look);
}

}  // namespace

int main() {
    const int lens[] = {0, 1, 11, 12, 13, 47, 48, 49, 95, 97, LIM_TILE - 1, LIM_TILE, LIM_TILE + 1, 2 * LIM_TILE + 47};
    const int looks[][2] = {{48, 1600}, {1, 1}, {LIM_MAX_L, 700}, {66, 2205}};
    for (const auto& t : looks) {
        for (int n : lens)
            for (int kind = 0; kind < 6; ++kind) check_single(kind, n, t[0], t[1]);
        check_packed(t[0], t[1]);
    }
    std::printf("limiter_host_check: %ld calls, %ld failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
