// Stand-alone check of csrc/eqstream.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/eqstream_host_check.cpp -o /tmp/eqstream_host_check && /tmp/eqstream_host_check
//
// (on x86-64 add -mfma: fma() then is one instruction instead of a call into libm, the same bits in a fifth of the time -- about
// three minutes under the sanitizers)
//
// It drives the host twin of the stream equaliser (eqs_init_host / eqs_push_host: the scalar routines the GPU kernels share) over
// 8, 32 and 192 kHz, 1, 3 and 6 sections, the edge lengths of the tests (around a run of 16 samples, a span of 8192, a chunk of two
// spans, three chunks and five) and noise, a tone, an impulse and a signal with a NaN and infinities.  Every stream is pushed whole
// and then cut in many ways -- one sample at a time, pushes of a run, a span and a chunk and one less and one more, one push that
// completes two chunks, random cuts with empty pushes, a flush carried by an empty push, in place and out of place -- always
// through the state the stream before left flushed, and every cutting must give the bytes and the last record of the whole.  The
// whole must be the bytes and the peaks of the clip twin eq_run_host over the same samples; with a NaN or an infinity among them,
// of the clip twin over the samples with zeros in their place, and the samples themselves at their places.  The state is a heap
// block of exactly eqs_state_bytes and every chunk and every `out` a heap block of exactly its length, so a read or write past any
// of them is a sanitizer report.  Exit status 0 only when all held.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "eqstream.h"

using namespace gsv;

namespace {

long g_calls = 0, g_streams = 0, g_fail = 0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;
const double kPi = 3.14159265358979323846;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

void expect(bool ok, const char* what, int rate, int count, int n, int kind) {
    if (ok) return;
    ++g_fail;
    std::fprintf(stderr, "FAILED: %s (rate %d, %d sections, n %d, signal %d)\n", what, rate, count, n, kind);
}

// kind 0 noise, 1 tone, 2 impulse, 3 noise with a NaN and infinities at a chunk's first and last sample and mid-run
std::vector<float> signal(int kind, int n, int rate) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 1: x[i] = (float)(0.5 * sin(2.0 * kPi * 60.0 * i / rate)); break;
            case 2: x[i] = i == 0 ? 1.f : 0.f; break;
            default: x[i] = (float)(2.0 * uniform() - 1.0); break;
        }
    }
    if (kind == 3) {
        const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                              -std::numeric_limits<float>::infinity()};
        const int at[6] = {0, n / 3, EQ_CHUNK - 1, EQ_CHUNK, EQ_CHUNK + EQ_SPAN + 7, n - 1};
        for (int k = 0; k < 6; ++k)
            if (at[k] >= 0 && at[k] < n) x[at[k]] = bad[k % 3];
    }
    return x;
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

struct Stream {
    std::vector<float> y;
    bool counts = true;
    int flags = 0;
    uint32_t pin = 0, pout = 0;         // the maxima of the per-push peaks
    EqsRecord last;
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
        EqsRecord rec;
        eqs_push_host(state, chunk.get(), n, k + 1 == cuts.size(), o, &rec);
        ++g_calls;
        s.counts = s.counts && rec.emitted == n && rec.total == (long long)at;
        s.y.insert(s.y.end(), o, o + n);
        s.flags |= rec.flags;
        s.pin = std::max(s.pin, loud_abs_bits(rec.peak_in));
        s.pout = std::max(s.pout, loud_abs_bits(rec.peak_out));
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

void check_stream(int rate, int count, int n, int kind, bool fine) {
    const std::vector<float> x = signal(kind, n, rate);
    const EqCoefs d = design(count, rate);
    if (!eq_coefs_ok(d)) { expect(false, "the design", rate, count, n, kind); return; }
    std::unique_ptr<unsigned char[]> state(new unsigned char[eqs_state_bytes()]);
    eqs_init_host(state.get(), d);
    const Stream whole = push_all(state.get(), x, {n}, false);
    expect(whole.counts && whole.last.total == n, "a flushed stream's length", rate, count, n, kind);

    // the clip twin over the same samples, zeros where they are not finite
    std::vector<float> z = x;
    bool bad = false;
    for (float& v : z)
        if (!eqs_finite(v)) { v = 0.f; bad = true; }
    const EqClip clip = {0, n, 0};
    EqLayout L;
    eq_layout(&clip, 1, 1, (size_t)n, true, &L, nullptr);
    std::unique_ptr<unsigned char[]> work(new unsigned char[L.bytes]);
    std::unique_ptr<float[]> want(new float[(size_t)n]);
    EqRecord crec;
    eq_run_host(z.data(), &clip, 1, &d, 1, want.get(), &crec, work.get());
    bool same = true, copied = true;
    for (int i = 0; i < n; ++i) {
        if (eqs_finite(x[i])) same = same && std::memcmp(&want[i], &whole.y[i], 4) == 0;
        else copied = copied && std::memcmp(&x[i], &whole.y[i], 4) == 0;
    }
    expect(same, "the stream differs from the clip", rate, count, n, kind);
    expect(copied, "a sample that is not finite was not copied", rate, count, n, kind);
    expect(whole.flags == (bad ? EQS_EQUALISED | EQS_NONFINITE | EQS_NONFINITE_EVER : EQS_EQUALISED), "flags", rate, count, n, kind);
    expect(loud_abs_bits(whole.last.peak_in_run) == loud_abs_bits(crec.peak_in), "peak_in_run is not the clip's peak_in", rate, count, n, kind);
    if (!bad) expect(loud_abs_bits(whole.last.peak_out_run) == loud_abs_bits(crec.peak_out), "peak_out_run is not the clip's", rate, count, n, kind);
    expect(eqs_finite(whole.last.peak_in_run) && eqs_finite(whole.last.peak_out_run), "a peak that is not finite", rate, count, n, kind);

    std::vector<std::vector<int>> cuttings;
    if (n <= 97) cuttings.push_back(cut_every(n, 1));
    for (int step : {EQ_R - 1, EQ_R, EQ_R + 1})
        if (fine) cuttings.push_back(cut_every(n, step));
    for (int step : {EQ_SPAN - 1, EQ_SPAN, EQ_SPAN + 1, EQ_CHUNK - 1, EQ_CHUNK, EQ_CHUNK + 1, 2 * EQ_CHUNK + 3}) cuttings.push_back(cut_every(n, step));
    for (int rep = 0; rep < 3; ++rep) {
        std::vector<int> c;
        for (int at = 0; at < n;) {
            int len = uniform() < 0.2 ? 0 : (int)(uniform() * (uniform() < 0.5 ? 40 : 3 * EQ_SPAN));
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
        expect(ok, "a cutting changed the bytes", rate, count, n, kind);
        expect(s.counts, "per-push counts", rate, count, n, kind);
        expect(s.flags == whole.flags && s.pin == whole.pin && s.pout == whole.pout, "per-push flags or peaks of a cutting", rate, count, n, kind);
        EqsRecord a = s.last, b = whole.last;       // the last push's own part differs with the cutting; the stream's does not
        a.emitted = b.emitted = 0;
        a.peak_in = b.peak_in = a.peak_out = b.peak_out = 0.f;
        a.flags &= ~EQS_NONFINITE; b.flags &= ~EQS_NONFINITE;
        expect(std::memcmp(&a, &b, sizeof a) == 0, "the stream's record under a cutting", rate, count, n, kind);
    }
}

}  // namespace

int main() {
    const int lens[] = {0, 1, EQ_R - 1, EQ_R, EQ_R + 1, 97, EQ_SPAN - 1, EQ_SPAN, EQ_SPAN + 1, EQ_CHUNK - 1, EQ_CHUNK, EQ_CHUNK + 1, 3 * EQ_CHUNK + 5,
                        5 * EQ_CHUNK + 3};
    const int rates[] = {32000, 8000, 192000};
    const int counts[] = {1, 3, 6};
    const auto t0 = std::chrono::steady_clock::now();
    for (int rate : rates)
        for (int count : counts)
            for (int n : lens)
                for (int kind = 0; kind < 4; ++kind)        // pushes of about a run: every stream of the voice design at 32 kHz, else the short ones
                    check_stream(rate, count, n, kind, (rate == 32000 && count == 3) || n <= EQ_SPAN + 1);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("eqstream_host_check: %ld streams, %ld pushes, %ld failures, %.1f s\n", g_streams, g_calls, g_fail, s);
    return g_fail || !g_calls ? 1 : 0;
}
