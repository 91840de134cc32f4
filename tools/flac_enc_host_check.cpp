// Stand-alone check of csrc/flacenc.h on the CPU, meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gsv-tts-lite_amd/csrc tools/flac_enc_host_check.cpp -o /tmp/flac_enc_host_check && /tmp/flac_enc_host_check
//
// It runs flac_encode_frame_host -- the serial encoder built from the scalar pieces the GPU kernel shares -- over the
// signal grid of the tests (tone + noise, noise past full scale, zeros, a constant, one outlier in silence, half-way
// ramps, NaN and infinities; lengths 1..2*4096+37; block sizes 16..4608; 16 and 24 bits).  Every frame's input is a heap
// block of exactly its samples and its output a heap block of exactly flac_enc_worst_bytes, the size the ABI demands per
// frame, so a read or write past either is a sanitizer report.  Each frame is then decoded by flac_decode_frame
// (csrc/flacdec.h) and must give the quantiser's integers, and the lane-split CRC-16 identity the kernel uses
// (crc(A || B) = crc(A) * x^(8 |B|) + crc(B)) is checked on every frame's bytes.  Exit status 0 only when all held.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "flacenc.h"

using namespace gsv;

namespace {

long g_files = 0, g_frames = 0, g_fail = 0;
uint64_t g_lcg = 0x9E3779B97F4A7C15ull;

double uniform() {          // [0, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_lcg >> 11) / 9007199254740992.0;
}

std::vector<float> signal(int kind, int n) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
        double v = 0;
        switch (kind) {
            case 0: v = 0.4 * sin(0.0446 * i) + 0.2 * sin(0.1967 * i) + 4e-4 * (uniform() - 0.5); break;
            case 1: v = 2.4 * (uniform() - 0.5); break;
            case 2: v = 0; break;
            case 3: v = 0.25 + 3.0 / 32768; break;
            case 4: v = i == n / 2 ? 1.0 : 0.0; break;
            case 5: v = (i - n / 2 + 0.5) / 32768.0; break;
            default: v = 0.3 * sin(0.069 * i) + 2e-3 * (uniform() - 0.5); break;
        }
        x[i] = (float)v;
    }
    if (kind == 6) {
        x[n / 3] = std::numeric_limits<float>::quiet_NaN();
        x[n / 2] = std::numeric_limits<float>::infinity();
        x[n - 1] = -std::numeric_limits<float>::infinity();
    }
    return x;
}

// the header of frame `number` of a mono fixed-blocking stream (rate code 0: from STREAMINFO)
int header(uint8_t* h, int bs, int bits, uint32_t number) {
    static const int kSizes[] = {0, 192, 576, 1152, 2304, 4608, 0, 0, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768};
    int code = bs <= 256 ? 6 : 7;
    for (int c = 1; c < 16; ++c)
        if (kSizes[c] == bs) code = c;
    int at = 0;
    h[at++] = 0xFF; h[at++] = 0xF8;
    h[at++] = (uint8_t)(code << 4);
    h[at++] = (uint8_t)((bits == 16 ? 4 : 6) << 1);
    if (number < 0x80) {
        h[at++] = (uint8_t)number;
    } else {
        int nb = 2;
        while (number >= (1u << (5 * nb + 1))) ++nb;
        h[at++] = (uint8_t)((0xFF << (8 - nb)) | (number >> (6 * (nb - 1))));
        for (int i = nb - 2; i >= 0; --i) h[at++] = (uint8_t)(0x80 | ((number >> (6 * i)) & 0x3F));
    }
    if (code == 6) h[at++] = (uint8_t)(bs - 1);
    if (code == 7) { h[at++] = (uint8_t)((bs - 1) >> 8); h[at++] = (uint8_t)(bs - 1); }
    unsigned c8 = 0;
    for (int i = 0; i < at; ++i) c8 = flac_crc8_byte(c8, h[i]);
    h[at++] = (uint8_t)c8;
    return at;
}

void check_clip(int kind, int n, int block, int bits) {
    const std::vector<float> x = signal(kind, n);
    ++g_files;
    for (int first = 0, k = 0; first < n; first += block, ++k) {
        const int bs = n - first < block ? n - first : block;
        uint8_t h[16];
        const int hl = header(h, bs, bits, (uint32_t)k * 70000u);        // numbers of 1..5 bytes
        std::unique_ptr<float[]> in(new float[(size_t)bs]);
        memcpy(in.get(), x.data() + first, (size_t)bs * sizeof(float));
        const uint32_t worst = flac_enc_worst_bytes(hl, bs, bits);
        std::unique_ptr<uint8_t[]> out(new uint8_t[worst]);
        FlacEncChoice ch;
        const uint32_t len = flac_encode_frame_host(in.get(), bs, bits, h, hl, out.get(), &ch);
        ++g_frames;
        if (len > worst || len < (uint32_t)hl + 3u) {
            fprintf(stderr, "kind %d n %d block %d bits %d frame %d: %u bytes (worst case %u)\n", kind, n, block, bits, k, len, worst);
            ++g_fail;
            continue;
        }
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);
        memcpy(exact.get(), out.get(), len);
        std::unique_ptr<int32_t[]> ints(new int32_t[(size_t)bs]);
        const int st = flac_decode_frame(exact.get(), len, 1, bits, bs, ints.get(), 0, false);
        bool same = st == FLAC_OK;
        for (int i = 0; same && i < bs; ++i) same = ints[i] == flac_enc_quantise(in[i], bits);
        if (!same) {
            fprintf(stderr, "kind %d n %d block %d bits %d frame %d: status %d or wrong integers (choice %d %d %d)\n", kind, n, block,
                    bits, k, st, ch.kind, ch.order, ch.porder);
            ++g_fail;
        }
        // the CRC-16 in 64 right-aligned chunks, combined as the kernel combines its lanes
        const uint32_t nbytes = len - 2, cb = (nbytes + 63) / 64, pad = 64 * cb - nbytes;
        unsigned crc[64], xp = 1;
        for (uint32_t j = 0; j < cb; ++j) xp = flac_crc16_byte(xp, 0);
        for (uint32_t l = 0; l < 64; ++l) {
            crc[l] = 0;
            for (uint32_t j = l * cb; j < (l + 1) * cb; ++j) crc[l] = flac_crc16_byte(crc[l], j < pad ? 0u : exact[j - pad]);
        }
        for (int s = 0; s < 6; ++s) {
            for (int l = 0; l < 64; l += 2 << s) crc[l] = flac_crc16_mulmod(crc[l], xp) ^ crc[l + (1 << s)];
            xp = flac_crc16_mulmod(xp, xp);
        }
        if (crc[0] != (((unsigned)exact[nbytes] << 8) | exact[nbytes + 1])) {
            fprintf(stderr, "kind %d n %d block %d bits %d frame %d: split CRC-16 %04x\n", kind, n, block, bits, k, crc[0]);
            ++g_fail;
        }
    }
}

}  // namespace

int main() {
    static const int kLengths[] = {1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 37};
    static const int kBlocks[] = {16, 192, 1000, 4096, 4608};
    const auto t0 = std::chrono::steady_clock::now();
    for (int bits = 16; bits <= 24; bits += 8)
        for (int block : kBlocks)
            for (int kind = 0; kind < 7; ++kind)
                for (int n : kLengths) check_clip(kind, n, block, bits);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%ld files, %ld frames, %ld failed expectations, %.2f s\n", g_files, g_frames, g_fail, s);
    return g_fail || !g_frames ? 1 : 0;
}
