// Stand-alone check of csrc/track.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/track_host_check.cpp -o /tmp/track_host_check && /tmp/track_host_check
//
// It drives the host twin of the real-time track output (track_init_host / track_push_host: the scalar routines the GPU
// kernels share) over the rate pairs, packet sizes, channel counts and signals of the tests, each stream cut into chunks
// at random -- lengths 0..700, runs of single samples, a flush of its own --, and compares the concatenated packets and
// every push's record with one push of the whole stream.  The state is a heap block of exactly track_state_bytes, every
// chunk a heap block of exactly its samples and every output a heap block of exactly track_out_capacity elements, the
// sizes the ABI states, so a read or write past any of them is a sanitizer report.  Exit status 0 only when all held.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "track.h"

using namespace gsv;

namespace {

long g_streams = 0, g_pushes = 0, g_fail = 0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

std::vector<float> signal(int kind, int n) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
        switch (kind) {
            case 0: x[i] = (float)(2.0 * uniform() - 1.0); break;
            case 1: x[i] = (float)(0.01 * sin(0.0432 * i)); break;
            case 2: x[i] = 0.f; break;
            default: x[i] = (float)(0.6 * uniform() - 0.3); break;
        }
    }
    if (kind == 3 && n > 2) {
        x[n / 3] = std::numeric_limits<float>::quiet_NaN();
        x[n / 2] = std::numeric_limits<float>::infinity();
        x[2 * n / 3] = -std::numeric_limits<float>::infinity();
    }
    return x;
}

struct Geo { int o, w, width, L, packet, channels; };

// one push through heap blocks of exactly the stated sizes; the packets are appended to `sink`
void push(unsigned char* state, const Geo& g, const float* x, int n, bool flush, std::vector<int16_t>* sink, int32_t* rec) {
    std::unique_ptr<float[]> in(new float[(size_t)n]);
    if (n) memcpy(in.get(), x, (size_t)n * sizeof(float));
    const long long cap = track_out_capacity(n, g.o, g.w, g.L, g.packet, g.channels);
    std::unique_ptr<int16_t[]> out(new int16_t[(size_t)cap]);
    track_push_host(state, in.get(), n, flush, out.get(), rec);
    ++g_pushes;
    const long long written = (long long)rec[0] * g.packet * g.channels;
    if (written > cap) {
        fprintf(stderr, "a push of %d samples names %lld elements, capacity %lld\n", n, written, cap);
        ++g_fail;
        return;
    }
    sink->insert(sink->end(), out.get(), out.get() + written);
}

void check_stream(int in_rate, int out_rate, int packet, int channels, int kind, int n) {
    Geo g;
    g.packet = packet; g.channels = channels;
    if (!track_params(in_rate, out_rate, &g.o, &g.w, &g.width)) { ++g_fail; return; }
    g.L = 2 * g.width + g.o;
    const size_t bytes = track_state_bytes(g.o, g.w, g.L, packet, channels);
    std::unique_ptr<unsigned char[]> state(new unsigned char[bytes]);
    track_init_host(state.get(), g.o, g.w, g.width, packet, channels);
    const std::vector<float> x = signal(kind, n);
    ++g_streams;
    std::vector<int16_t> whole, cut;
    int32_t rec[4];
    push(state.get(), g, x.data(), n, true, &whole, rec);
    const long long M = track_total(n, g.o, g.w);
    if (rec[1] != M || rec[0] != (M + packet - 1) / packet || rec[2] != 0 || rec[3] != rec[0] * (long long)packet - M) {
        fprintf(stderr, "%d -> %d packet %d: one-shot record %d %d %d %d for %lld outputs\n", in_rate, out_rate, packet, rec[0], rec[1],
                rec[2], rec[3], M);
        ++g_fail;
    }
    // the same state again (a flush leaves it fresh), cut at random
    for (int round = 0; round < 3; ++round) {
        cut.clear();
        long long produced = 0;
        int at = 0, pushes = 0;
        const bool own_flush = round == 2;
        while (at < n) {
            int len = round == 1 && pushes < 40 ? 1 : (int)(uniform() * 701);
            if (uniform() < 0.1) len = 0;
            if (len > n - at) len = n - at;
            const bool last = at + len == n && !own_flush;
            push(state.get(), g, x.data() + at, len, last, &cut, rec);
            produced += rec[1];
            if (!last && produced != track_avail(at + len, g.o, g.w, g.width)) {
                fprintf(stderr, "%d -> %d: %lld outputs after %d samples, the rule says %lld\n", in_rate, out_rate, produced, at + len,
                        track_avail(at + len, g.o, g.w, g.width));
                ++g_fail;
            }
            at += len;
            ++pushes;
        }
        if (own_flush || n == 0) {
            push(state.get(), g, nullptr, 0, true, &cut, rec);
            produced += rec[1];
        }
        if (produced != M || cut != whole) {
            fprintf(stderr, "%d -> %d packet %d channels %d kind %d n %d round %d: the chunked stream differs (%zu / %zu elements)\n", in_rate,
                    out_rate, packet, channels, kind, n, round, cut.size(), whole.size());
            ++g_fail;
        }
    }
}

}  // namespace

int main() {
    static const int kPairs[][2] = {{32000, 48000}, {32000, 16000}, {32000, 8000}, {32000, 44100}, {32000, 24000},
                                    {32000, 32000}, {48000, 32000}, {32000, 125}};
    static const int kPackets[] = {960, 7, 1};
    static const int kLengths[] = {0, 1, 5, 333, 2000, 5003};
    const auto t0 = std::chrono::steady_clock::now();
    for (const auto& pair : kPairs)
        for (int packet : kPackets)
            for (int channels = 1; channels <= 2; ++channels)
                for (int kind = 0; kind < 4; ++kind)
                    for (int n : kLengths) check_stream(pair[0], pair[1], packet, channels, kind, n);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%ld streams, %ld pushes, %ld failed expectations, %.2f s\n", g_streams, g_pushes, g_fail, s);
    return g_fail || !g_pushes ? 1 : 0;
}
