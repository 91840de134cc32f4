// Stand-alone check of csrc/limstream.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/limstream_host_check.cpp -o /tmp/limstream_host_check && /tmp/limstream_host_check
//
// It drives the host twin of the stream limiter (lims_init_host / lims_push_host: the scalar routines the GPU kernels share) over
// the edge lengths of the tests with a sine above the ceiling, clicks at both ends and on a tile edge, noise, a quiet sine and a NaN;
// look-aheads of 1, 48, 66 and the longest the ABI takes.  Every stream is pushed whole and then cut in many ways -- one sample at
// a time, pushes of D - 1, D and D + 1, cuts around a tile edge, random cuts with empty pushes, a flush carried by an empty push --
// and every cutting must give the bytes and the per-push counts of the whole.  The state is a heap block of exactly
// lims_state_bytes, every chunk a heap block of exactly its length and every `out` one of exactly n + D floats, so a read or write
// past any of them is a sanitizer report.  It also holds the output against the clip twin's gain (fl(g x), bit for bit, where the
// clip was limited and fl(L fl(1 / L)) == 1; x itself where it was not), |y| <= T (1 + 2^-22), and a second stream through the
// flushed state against a fresh state.  Exit status 0 only when all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "limstream.h"

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

struct Stream {
    std::vector<float> y;
    std::vector<int> counts;
    int flags = 0;
    LimsRecord last;
};

// the stream cut at `cuts` (lengths; the last push flushes) through `state`
Stream push_all(unsigned char* state, const std::vector<float>& x, const std::vector<int>& cuts, int look) {
    Stream s;
    size_t at = 0;
    for (size_t k = 0; k < cuts.size(); ++k) {
        const int n = cuts[k];
        std::unique_ptr<float[]> chunk(new float[(size_t)n]), out(new float[(size_t)n + lims_delay(look)]);
        if (n) std::memcpy(chunk.get(), x.data() + at, (size_t)n * sizeof(float));
        at += (size_t)n;
        LimsRecord rec;
        lims_push_host(state, chunk.get(), n, k + 1 == cuts.size(), out.get(), &rec);
        ++g_calls;
        s.y.insert(s.y.end(), out.get(), out.get() + rec.emitted);
        s.counts.push_back(rec.emitted);
        s.flags |= rec.flags;
        s.last = rec;
    }
    return s;
}

std::vector<int> cut_every(int n, int step) {
    std::vector<int> c;
    for (int at = 0; at < n; at += step) c.push_back(n - at < step ? n - at : step);
    if (c.empty()) c.push_back(0);
    return c;
}

void check_stream(int kind, int n, int look, int rel) {
    const std::vector<float> x = signal(kind, n);
    const size_t bytes = lims_state_bytes(look);
    std::unique_ptr<unsigned char[]> state(new unsigned char[bytes]);
    lims_init_host(state.get(), -1.f, look, rel);
    const int D = lims_delay(look);
    const Stream whole = push_all(state.get(), x, {n}, look);
    expect((int)whole.y.size() == n && whole.last.total == n, "a flushed stream's length", n, kind, look);
    expect(((whole.flags & LIMS_NONFINITE) != 0) == (kind == 5 && n > 0), "nonfinite flag", n, kind, look);

    std::vector<std::vector<int>> cuttings;
    if (n <= 97) cuttings.push_back(cut_every(n, 1));
    for (int step : {D - 1, D, D + 1, LIM_TILE - 1, LIM_TILE, LIM_TILE + 1})
        if (step >= 1) cuttings.push_back(cut_every(n, step));
    for (int rep = 0; rep < 3; ++rep) {
        std::vector<int> c;
        for (int at = 0; at < n;) {
            int len = uniform() < 0.2 ? 0 : (int)(uniform() * (uniform() < 0.5 ? 40 : 1500));
            if (len > n - at) len = n - at;
            c.push_back(len);
            at += len;
        }
        c.push_back(0);             // the flush is an empty push
        cuttings.push_back(c);
    }
    for (const auto& cuts : cuttings) {
        // through the state the stream before left flushed: it equals a fresh one
        const Stream s = push_all(state.get(), x, cuts, look);
        bool ok = s.y.size() == whole.y.size() && (n == 0 || std::memcmp(s.y.data(), whole.y.data(), (size_t)n * 4) == 0);
        expect(ok, "a cutting changed the bytes", n, kind, look);
        long long seen = 0, emitted = 0;
        bool counts = true;
        for (size_t k = 0; k < cuts.size(); ++k) {
            seen += cuts[k];
            const long long due = k + 1 == cuts.size() ? seen : (seen > D ? seen - D : 0);
            counts = counts && s.counts[k] == due - emitted;
            emitted = due;
        }
        expect(counts, "per-push counts", n, kind, look);
        expect(s.last.total == n && (s.flags & ~LIMS_LIMITED_EVER) == (whole.flags & ~LIMS_LIMITED_EVER), "records of a cutting", n, kind,
               look);
    }

    const float T = (float)std::pow(10.0, -1.0 / 20.0);
    bool bound = true;
    for (int i = 0; i < n; ++i) bound = bound && (x[i] != x[i] || std::fabs(whole.y[i]) <= T * (1.f + 2.4e-7f));
    expect(bound, "|y| above T (1 + 2^-22)", n, kind, look);
    if (kind == 5 || n == 0) return;
    // the clip twin's stage array
    const LimClip clip = {0, n, -1.f};
    LimLayout L;
    lim_layout(&clip, 1, (size_t)n, true, &L, nullptr);
    std::unique_ptr<unsigned char[]> work(new unsigned char[L.bytes]);
    std::unique_ptr<float[]> out(new float[(size_t)n]);
    LimRecord rec;
    lim_run_host(x.data(), &clip, 1, look, rel, out.get(), &rec, work.get());
    const float* g = reinterpret_cast<const float*>(work.get() + L.g_off);
    const bool limited = rec.flags & LIM_LIMITED;
    expect(limited == ((whole.flags & LIMS_LIMITED) != 0), "limited as the clip is", n, kind, look);
    if ((float)look * (1.f / (float)look) != 1.f && limited) return;
    bool same = true;
    for (int i = 0; i < n; ++i) {
        const float want = limited ? g[i] * x[i] : x[i];
        same = same && std::memcmp(&want, &whole.y[i], 4) == 0;
    }
    expect(same, "the stream differs from fl(g x) of the clip", n, kind, look);
}

}  // namespace

int main() {
    const int lens[] = {0, 1, 11, 12, 13, 47, 48, 49, 95, 97, LIM_TILE - 1, LIM_TILE, LIM_TILE + 1, 2 * LIM_TILE + 47, 4 * LIM_TILE + 47};
    const int looks[][2] = {{48, 1600}, {1, 1}, {LIM_MAX_L, 700}, {66, 2205}};
    for (const auto& t : looks)
        for (int n : lens)
            for (int kind = 0; kind < 6; ++kind) check_stream(kind, n, t[0], t[1]);
    std::printf("limstream_host_check: %ld calls, %ld failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
