// Stand-alone check of csrc/cmpstream.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/cmpstream_host_check.cpp -o /tmp/cmpstream_host_check && /tmp/cmpstream_host_check
//
// (on x86-64 add -mfma: fma() then is one instruction instead of a call into libm, the same bits in a fraction of the time)
//
// It drives the host twin of the stream compressor (cms_init_host / cms_push_host: the scalar routines the GPU kernels share) over
// 8, 32 and 48 kHz, four parameter sets (the "voice" preset, a fast 20 : 1, a slow 2 : 1 with makeup, a limiter's curve), the edge
// lengths of the tests (around a run of 16 samples, a span of 8192, a chunk of two spans, two chunks + a span + 5, three chunks + 5)
// and noise, a gated tone whose attacks and releases cross the span and chunk edges, a square wave and the gated tone with NaNs
// and infinities at run, span and chunk edges.  Every stream is pushed whole and then cut in many ways -- one sample at a time,
// pushes of a run, a span and a chunk and one less and one more, one push that completes two chunks, random cuts with empty
// pushes, a flush carried by an empty push, in place and out of place -- always through the state the stream before left flushed,
// and every cutting must give the bytes and the last record of the whole.  The whole must be the bytes, the peaks and the smallest
// gain of the clip twin cmp_run_host over the same samples; with a NaN or an infinity among them, the bytes of the clip twin over
// the samples with zeros in their place, and the samples themselves at their places.  The state is a heap block of exactly
// cms_state_bytes and every chunk and every `out` a heap block of exactly its length, so a read or write past any of them is a
// sanitizer report.  Exit status 0 only when all held.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "cmpstream.h"

using namespace gsv;

namespace {

long g_calls = 0, g_streams = 0, g_fail = 0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;
const double kPi = 3.14159265358979323846;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

void expect(bool ok, const char* what, int rate, int set, int n, int kind) {
    if (ok) return;
    ++g_fail;
    std::fprintf(stderr, "FAILED: %s (rate %d, parameter set %d, n %d, signal %d)\n", what, rate, set, n, kind);
}

// kind 0 noise, 1 a 220 Hz tone gated every 3001 samples between 0.9 and 0.01, 2 a square wave, 3 the gated tone with NaNs and
// infinities at a run's, a span's and a chunk's first and last sample and mid-run
std::vector<float> signal(int kind, int n, int rate) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 0: x[i] = (float)(2.0 * uniform() - 1.0); break;
            case 2: x[i] = (i / 32) % 2 == 0 ? 1.f : -1.f; break;
            default: x[i] = (float)(((i / 3001) % 2 == 0 ? 0.9 : 0.01) * sin(2.0 * kPi * 220.0 * i / rate)); break;
        }
    }
    if (kind == 3) {
        const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                              -std::numeric_limits<float>::infinity()};
        const int at[10] = {0, CMP_R - 1, CMP_R, n / 3, CMP_SPAN - 1, CMP_SPAN, CMP_CHUNK - 1, CMP_CHUNK, CMP_CHUNK + CMP_SPAN + 7, n - 1};
        for (int k = 0; k < 10; ++k)
            if (at[k] >= 0 && at[k] < n) x[at[k]] = bad[k % 3];
    }
    return x;
}

// set 0 "voice", 1 fast, 2 slow with makeup, 3 a limiter's curve: (threshold dB, ratio, attack ms, release ms, makeup dB)
CmpParams params(int set, int rate) {
    const double sets[4][5] = {{-18.0, 3.5, 1.0, 100.0, 0.0}, {-30.0, 20.0, 0.1, 5.0, 0.0}, {-6.0, 2.0, 30.0, 1000.0, 3.0},
                               {-18.0, std::numeric_limits<double>::infinity(), 1.0, 100.0, 0.0}};
    const double* s = sets[set];
    CmpParams d;
    d.attack = exp(-2.0 * kPi * 1000.0 / (rate * s[2]));
    d.release = exp(-2.0 * kPi * 1000.0 / (rate * s[3]));
    d.threshold = pow(10.0, s[0] / 20.0);
    d.slope = 1.0 / s[1] - 1.0;
    d.makeup = pow(10.0, s[4] / 20.0);
    return d;
}

struct Stream {
    std::vector<float> y;
    bool counts = true;
    int flags = 0;
    uint32_t pin = 0, pout = 0, gmin = CMP_ONE_BITS;    // the extrema of the per-push values
    CmsRecord last;
};

// the stream cut at `cuts` (lengths; the last push flushes) through `state`; in place on every other push when asked
Stream push_all(unsigned char* state, const std::vector<float>& x, const std::vector<int>& cuts, bool inplace) {
    Stream s;
    size_t at = 0;
    memset(&s.last, 0, sizeof s.last);
    for (size_t k = 0; k < cuts.size(); ++k) {
        const int n = cuts[k];
        std::unique_ptr<float[]> chunk(new float[(size_t)n]), out(new float[(size_t)n]);
        if (n) std::memcpy(chunk.get(), x.data() + at, (size_t)n * sizeof(float));
        at += (size_t)n;
        float* o = inplace && (k & 1) == 0 ? chunk.get() : out.get();
        CmsRecord rec;
        memset(&rec, 0, sizeof rec);
        cms_push_host(state, chunk.get(), n, k + 1 == cuts.size(), o, &rec);
        ++g_calls;
        s.counts = s.counts && rec.emitted == n && rec.total == (long long)at;
        s.counts = s.counts && ((rec.flags & CMS_COMPRESSED) != 0) == (rec.min_gain < 1.f);
        s.y.insert(s.y.end(), o, o + n);
        s.flags |= rec.flags & ~CMS_COMPRESSED;
        s.pin = std::max(s.pin, loud_abs_bits(rec.peak_in));
        s.pout = std::max(s.pout, loud_abs_bits(rec.peak_out));
        s.gmin = std::min(s.gmin, loud_abs_bits(rec.min_gain));
        s.last = rec;
    }
    ++g_streams;
    return s;
}

std::vector<int> cut_every(int n, int step) {
    std::vector<int> c;
    for (int at = 0; at < n; at += step) c.push_back(n - at < step ? n - at : step);
    if (c.empty()) c.push_back(0);
    return c;
}

void check_stream(int rate, int set, int n, int kind, bool fine) {
    const std::vector<float> x = signal(kind, n, rate);
    const CmpParams d = params(set, rate);
    if (!cmp_params_ok(d)) { expect(false, "the parameters", rate, set, n, kind); return; }
    std::unique_ptr<unsigned char[]> state(new unsigned char[cms_state_bytes()]);
    cms_init_host(state.get(), d);
    const Stream whole = push_all(state.get(), x, {n}, false);
    expect(whole.counts && whole.last.total == n, "a flushed stream's length", rate, set, n, kind);

    // the clip twin over the same samples, zeros where they are not finite
    std::vector<float> z = x;
    bool bad = false;
    for (float& v : z)
        if (!cms_finite(v)) { v = 0.f; bad = true; }
    const CmpClip clip = {0, n, 0};
    CmpLayout L;
    cmp_layout(&clip, 1, 1, (size_t)n, true, &L, nullptr);
    std::unique_ptr<unsigned char[]> work(new unsigned char[L.bytes]);
    std::unique_ptr<float[]> want(new float[(size_t)n]);
    CmpRecord crec;
    cmp_run_host(z.data(), &clip, 1, &d, 1, want.get(), &crec, work.get());
    bool same = true, copied = true;
    for (int i = 0; i < n; ++i) {
        if (cms_finite(x[i])) same = same && std::memcmp(&want[i], &whole.y[i], 4) == 0;
        else copied = copied && std::memcmp(&x[i], &whole.y[i], 4) == 0;
    }
    expect(same, "the stream differs from the clip", rate, set, n, kind);
    expect(copied, "a sample that is not finite was not copied", rate, set, n, kind);
    expect(whole.flags == (bad ? CMS_STREAM | CMS_NONFINITE | CMS_NONFINITE_EVER : CMS_STREAM), "flags", rate, set, n, kind);
    expect(loud_abs_bits(whole.last.peak_in_run) == loud_abs_bits(crec.peak_in), "peak_in_run is not the clip's peak_in", rate, set, n, kind);
    if (!bad) {
        expect(loud_abs_bits(whole.last.peak_out_run) == loud_abs_bits(crec.peak_out), "peak_out_run is not the clip's", rate, set, n, kind);
        expect(loud_abs_bits(whole.last.min_gain_run) == loud_abs_bits(crec.min_gain), "min_gain_run is not the clip's", rate, set, n, kind);
    } else {        // the gains at the samples left out are not counted
        expect(whole.last.min_gain_run >= crec.min_gain, "min_gain_run below the clip's", rate, set, n, kind);
    }
    expect(cms_finite(whole.last.peak_in_run) && cms_finite(whole.last.peak_out_run) && cms_finite(whole.last.min_gain_run),
           "a record value that is not finite", rate, set, n, kind);

    std::vector<std::vector<int>> cuttings;
    if (n <= 97) cuttings.push_back(cut_every(n, 1));
    for (int step : {CMP_R - 1, CMP_R, CMP_R + 1})
        if (fine) cuttings.push_back(cut_every(n, step));
    for (int step : {CMP_SPAN - 1, CMP_SPAN, CMP_SPAN + 1, CMP_CHUNK - 1, CMP_CHUNK, CMP_CHUNK + 1, 2 * CMP_CHUNK + 3})
        cuttings.push_back(cut_every(n, step));
    for (int rep = 0; rep < 3; ++rep) {
        std::vector<int> c;
        for (int at = 0; at < n;) {
            int len = uniform() < 0.2 ? 0 : (int)(uniform() * (uniform() < 0.5 ? 40 : 3 * CMP_SPAN));
            if (len > n - at) len = n - at;
            c.push_back(len);
            at += len;
        }
        c.push_back(0);             // the flush is an empty push
        cuttings.push_back(c);
    }
    int turn = 0;
    for (const auto& cuts : cuttings) {
        // through the state the stream before left flushed: it equals a fresh one
        const Stream s = push_all(state.get(), x, cuts, (turn++ & 1) != 0);
        const bool ok = s.y.size() == whole.y.size() && (n == 0 || std::memcmp(s.y.data(), whole.y.data(), (size_t)n * 4) == 0);
        expect(ok, "a cutting changed the bytes", rate, set, n, kind);
        expect(s.counts, "per-push counts", rate, set, n, kind);
        expect(s.flags == whole.flags && s.pin == whole.pin && s.pout == whole.pout && s.gmin == whole.gmin,
               "per-push flags, peaks or smallest gain of a cutting", rate, set, n, kind);
        CmsRecord a = s.last, b = whole.last;       // the last push's own part differs with the cutting; the stream's does not
        a.emitted = b.emitted = 0;
        a.peak_in = b.peak_in = a.peak_out = b.peak_out = 0.f;
        a.min_gain = b.min_gain = 1.f;
        a.flags &= ~(CMS_NONFINITE | CMS_COMPRESSED); b.flags &= ~(CMS_NONFINITE | CMS_COMPRESSED);
        expect(std::memcmp(&a, &b, sizeof a) == 0, "the stream's record under a cutting", rate, set, n, kind);
    }
}

}  // namespace

int main() {
    const int lens[] = {0, 1, CMP_R - 1, CMP_R, CMP_R + 1, 97, CMP_SPAN - 1, CMP_SPAN, CMP_SPAN + 1, CMP_CHUNK - 1, CMP_CHUNK, CMP_CHUNK + 1,
                        2 * CMP_CHUNK + CMP_SPAN + 5, 3 * CMP_CHUNK + 5};
    const int rates[] = {32000, 8000, 48000};
    const auto t0 = std::chrono::steady_clock::now();
    for (int rate : rates)
        for (int set = 0; set < 4; ++set)
            for (int n : lens)
                for (int kind = 0; kind < 4; ++kind)    // pushes of about a run: the voice set at 32 kHz up to a span + 1, else up to 97 samples
                    check_stream(rate, set, n, kind, n <= 97 || (rate == 32000 && set == 0 && n <= CMP_SPAN + 1));
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("cmpstream_host_check: %ld streams, %ld pushes, %ld failures, %.1f s\n", g_streams, g_calls, g_fail, s);
    return g_fail || !g_calls ? 1 : 0;
}
