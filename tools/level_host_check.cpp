// Stand-alone check of csrc/level.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/level_host_check.cpp -o /tmp/level_host_check && /tmp/level_host_check
//
// It drives the host twin of the stream leveller (level_init_host / level_push_host: the scalar routines the GPU kernels share)
// over rates from 4 to 192 kHz -- runs of 1 to 16 samples, hops of one, two and three spans, hops of unequal length at 11 025 Hz --
// and over noise, a tone, silence, a stepped signal and one with a NaN and an infinity.  The state is a heap block of exactly
// level_state_bytes, every chunk and every output a heap block of exactly the push's samples and the record a heap block of
// one record, so a read or write past any of them is a sanitizer report.  It holds the twin
//   - to a plain serial filter with plain sums over the same hops: counts equal, zbar and every knot gain within 1e-6 LU (what
//     tools/loudness_host_check.cpp asks of the same scan; the worst case found is printed);
//   - to itself under random cuts of the stream, in place and out of place: samples, the final record (but for the gain of the
//     last push's first sample, which is wherever that push began) and state bytes equal;
//   - to the history's capacity: a stream past max_seconds freezes with GSV_LEVEL_FULL and writes no further block.
// Exit status 0 only when all held.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "level.h"

using namespace gsv;

namespace {

long g_pushes = 0, g_streams = 0, g_fail = 0;
double g_worst_lu = 0.0;
const double kLu = 1e-6;     // LU
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

std::vector<float> signal(int kind, int n, int rate) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 1: x[i] = (float)(0.5 * sin(2.0 * 3.14159265358979323846 * 60.0 * i / rate)); break;
            case 2: x[i] = 0.f; break;
            case 3: x[i] = (float)((0.6 * uniform() - 0.3) * (i / (rate / 2) % 2 ? 1e-5 : 1.0)); break;      // loud and gated halves
            default: x[i] = (float)(0.6 * uniform() - 0.3); break;
        }
    }
    if (kind == 4 && n > 2) {
        x[n / 2] = std::numeric_limits<float>::quiet_NaN();
        x[2 * n / 3] = std::numeric_limits<float>::infinity();
    }
    return x;
}

void fail(const char* what, int rate, int kind, long at) {
    fprintf(stderr, "rate %d kind %d at %ld: %s\n", rate, kind, at, what);
    ++g_fail;
}

struct Config { double target, seed, seed_blocks, slew, max_gain; float peak_limit; int max_seconds; };

struct Stream {
    std::unique_ptr<unsigned char[]> state;
    size_t bytes;
    std::vector<float> out;
    LevelRecord last;
    std::vector<double> knots;
};

// the stream x pushed in the given lengths, the last with the flush; every buffer a heap block of its exact size
Stream run(const std::vector<float>& x, int rate, const Config& c, const std::vector<int>& plan, bool in_place) {
    Stream s;
    const int cap_blocks = level_cap_blocks(rate, c.max_seconds);
    s.bytes = level_state_bytes(cap_blocks + 3, cap_blocks, level_ring_len(rate));
    s.state.reset(new unsigned char[s.bytes]);
    level_init_host(s.state.get(), rate, c.target, c.seed, c.seed_blocks, c.slew, c.max_gain, c.peak_limit, c.max_seconds);
    size_t at = 0;
    for (size_t i = 0; i < plan.size(); ++i) {
        const int n = plan[i];
        std::unique_ptr<float[]> chunk(new float[(size_t)n]), other(new float[(size_t)n]);
        std::unique_ptr<LevelRecord> rec(new LevelRecord);
        if (n) memcpy(chunk.get(), x.data() + at, (size_t)n * sizeof(float));
        float* out = in_place ? chunk.get() : other.get();
        const bool flush = i + 1 == plan.size();
        level_push_host(s.state.get(), chunk.get(), n, flush, out, rec.get());
        ++g_pushes;
        if (!in_place && n && memcmp(chunk.get(), x.data() + at, (size_t)n * sizeof(float))) fail("the chunk was changed", rate, 0, (long)at);
        s.out.insert(s.out.end(), out, out + n);
        s.last = *rec;
        at += (size_t)n;
    }
    LevelHeader h;
    memcpy(&h, s.state.get(), sizeof h);
    const double* A = reinterpret_cast<const double*>(s.state.get() + level_knots_off());
    s.knots.assign(A, A + h.K + 1);
    ++g_streams;
    return s;
}

std::vector<int> random_plan(int n, int hop) {
    std::vector<int> plan;
    int left = n;
    while (left) {
        int m = (int)(uniform() * (2.5 * hop));
        if (uniform() < 0.15) m = uniform() < 0.5 ? 0 : 1;
        if (m > left) m = left;
        plan.push_back(m);
        left -= m;
    }
    if (plan.empty()) plan.push_back(0);
    return plan;
}

// the definition with a plain serial filter and plain sums -> the knots, and the final counts and zbar
void serial(const std::vector<float>& x, int rate, const Config& c, std::vector<double>* knots, int* blocks, int* above, int* kept, double* zbar,
            bool* frozen) {
    const LoudParams p = loud_params(rate, c.peak_limit);
    const bool seeded = c.seed == c.seed;
    const double k = pow(10.0, (c.target + 0.691) / 10.0), G = pow(10.0, c.max_gain / 20.0), r = pow(10.0, c.slew * 0.1 / 20.0);
    const double w = seeded ? c.seed_blocks : 0.0, seed_z = seeded ? pow(10.0, (c.seed + 0.691) / 10.0) : 0.0;
    const int cap_blocks = level_cap_blocks(rate, c.max_seconds);
    auto next = [&](double A, int kp, double zb, double peak) {
        double d = 1.0;
        if (w + kp > 0) d = sqrt(k / ((w * seed_z + kp * zb) / (w + kp)));
        d = std::min(std::max(d, 1.0 / G), G);
        if (peak > 0) d = std::min(d, (double)c.peak_limit / peak);
        return std::min(std::max(d, A / r), A * r);
    };
    double A0 = seeded ? std::min(std::max(sqrt(k / seed_z), 1.0 / G), G) : 1.0;
    knots->assign(1, A0);
    knots->push_back(next(A0, 0, 0.0, 0.0));
    LoudState st = {{0, 0, 0, 0}};
    std::vector<double> S, z;
    double peak = 0.0;
    *blocks = *above = *kept = 0; *zbar = 0.0; *frozen = false;
    for (int h = 0;; ++h) {
        const long long lo = level_knot(h, rate), hi = level_knot(h + 1, rate);
        if (hi > (long long)x.size()) break;
        bool finite = true;
        for (long long i = lo; i < hi; ++i) finite = finite && std::isfinite(x[(size_t)i]);
        if (!finite) { *frozen = true; break; }
        double acc = 0.0;
        for (long long i = lo; i < hi; ++i) {
            const double y = loud_step(p, st, x[(size_t)i]);
            acc += y * y;
            peak = std::max(peak, (double)fabsf(x[(size_t)i]));
        }
        S.push_back(acc);
        const int n = (int)S.size();
        if (n >= 4) z.push_back((S[n - 4] + S[n - 3] + S[n - 2] + S[n - 1]) / p.gate_len);
        double sa = 0, sk = 0;
        int na = 0, nk = 0;
        for (double v : z) if (v >= p.abs_thr) { sa += v; ++na; }
        const double rel = na ? 0.1 * sa / na : 0.0;
        if (na) for (double v : z) if (v > rel && v > p.abs_thr) { sk += v; ++nk; }
        *blocks = (int)z.size(); *above = na; *kept = nk; *zbar = nk ? sk / nk : 0.0;
        knots->push_back(next(knots->back(), nk, *zbar, peak));
        if ((int)z.size() == cap_blocks) { *frozen = true; break; }
    }
}

void check(int rate, int kind, double seconds, const Config& c) {
    const int n = (int)(seconds * rate), hop = (int)level_knot(1, rate);
    const std::vector<float> x = signal(kind, n, rate);
    const Stream one = run(x, rate, c, {n}, false);
    // against the serial definition
    std::vector<double> knots;
    int blocks, above, kept;
    double zbar;
    bool frozen;
    serial(x, rate, c, &knots, &blocks, &above, &kept, &zbar, &frozen);
    if (one.last.blocks != blocks || one.last.above_abs != above || one.last.kept != kept) fail("counts differ from the serial filter", rate, kind, blocks);
    auto lu = [](double a, double b) { const double d = fabs(10.0 * log10(a / b)); g_worst_lu = d > g_worst_lu ? d : g_worst_lu; return d; };
    if ((zbar == 0) != (one.last.zbar == 0) || (zbar > 0 && lu(one.last.zbar, zbar) > kLu)) fail("zbar differs from the serial filter", rate, kind, 0);
    if (knots.size() != one.knots.size()) fail("knot count differs from the serial filter", rate, kind, (long)one.knots.size());
    else
        for (size_t h = 0; h < knots.size(); ++h)
            if (lu(one.knots[h] * one.knots[h], knots[h] * knots[h]) > kLu) { fail("a knot gain differs from the serial filter", rate, kind, (long)h); break; }
    const bool is_frozen = (one.last.flags & (LEVEL_NONFINITE | LEVEL_FULL)) != 0;
    if (is_frozen != frozen) fail("frozen / not frozen disagrees with the serial filter", rate, kind, one.last.flags);
    if (kind == 2)
        for (int i = 0; i < n; ++i)
            if (one.out[(size_t)i] != 0.f) { fail("silence did not come back as silence", rate, kind, i); break; }
    // against itself under other cuts
    for (int rep = 0; rep < 3; ++rep) {
        std::vector<int> plan = rep == 0 ? std::vector<int>{hop - 1, 1, 1, hop - 1, hop + 1, n - 3 * hop - 2 > 0 ? n - 3 * hop - 2 : 0} : random_plan(n, hop);
        if (rep == 0) {
            long sum = 0;
            for (int v : plan) sum += v;
            if (sum != n) plan = {n / 2, n - n / 2};
        }
        const Stream cut = run(x, rate, c, plan, rep % 2 == 1);
        if (cut.out.size() != one.out.size() || memcmp(cut.out.data(), one.out.data(), one.out.size() * sizeof(float))) fail("samples depend on the cut", rate, kind, rep);
        LevelRecord a = cut.last, b = one.last;
        a.gain_first = b.gain_first = 0.f;
        if (memcmp(&a, &b, sizeof(LevelRecord))) fail("the final record depends on the cut", rate, kind, rep);
        if (cut.bytes != one.bytes || memcmp(cut.state.get(), one.state.get(), one.bytes)) fail("the state bytes depend on the cut", rate, kind, rep);
    }
}

}  // namespace

int main() {
    static const int kRates[] = {4000, 8000, 11025, 32000, 44100, 96000, 192000};
    const auto t0 = std::chrono::steady_clock::now();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int rate : kRates) {
        const double seconds = rate > 50000 ? 1.23 : 2.57;
        for (int kind = 0; kind < 5; ++kind) {
            check(rate, kind, seconds, Config{-18.0, nan, 10.0, 10.0, 20.0, 1.f, 600});
            check(rate, kind, seconds, Config{-23.0, -30.0, 10.0, 20.0, 12.0, 0.5f, 1});       // seeded, clamping, a history of 7 blocks
        }
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%ld streams, %ld pushes, %ld failed expectations, worst %.3g LU from the serial filter, %.2f s\n", g_streams, g_pushes, g_fail, g_worst_lu, s);
    return g_fail || !g_streams ? 1 : 0;
}
