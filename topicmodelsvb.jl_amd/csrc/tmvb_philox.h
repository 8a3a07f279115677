// tmvb_philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), plain C++ for host and device.
//
// A counter-based generator: the 128 random bits are a pure function of a 128-bit counter and a 64-bit key.  The corpus generator
// (tmvb_gencorp.hip) keys it with the caller's seed and counts with (global document index, stage, draw index), so no random number
// depends on the launch geometry, on how many documents a call generates, or on where the call's first document lies.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TMVB_HD __host__ __device__
#else
#define TMVB_HD
#endif

struct tmvb_philox4 {
    uint32_t x[4];
};

TMVB_HD inline tmvb_philox4 tmvb_philox4x32_10_raw(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    return tmvb_philox4{{c0, c1, c2, c3}};
}

// The stages of the generative process: one counter sub-space each (counter word 2; the topic index of a per-topic draw rides in its upper bits).
// TMVB_RNG_SPLIT is the held-out token split (tmvb_heldout.hip): draw index = Philox block of a document's token occurrences.
// TMVB_RNG_RSPLIT_ENTRY / _DOCUMENT are the split of the reader lists (tmvb_recranks.hip): draw index = Philox block of a document's reader entries / 0.
enum : uint32_t { TMVB_RNG_POISSON = 0, TMVB_RNG_GAMMA = 1, TMVB_RNG_BOOST = 2, TMVB_RNG_NORMAL = 3, TMVB_RNG_TOKEN = 4, TMVB_RNG_SPLIT = 5,
                  TMVB_RNG_RSPLIT_ENTRY = 6, TMVB_RNG_RSPLIT_DOCUMENT = 7, TMVB_RNG_KMEANS = 8, TMVB_RNG_MAP = 9 };

// TMVB_RNG_KMEANS is the k-means++ seeding (tmvb_kmeans.hip): "document" = the seeding round j, draw index 0.
// TMVB_RNG_MAP is the random start of the document map (tmvb_docmap.hip): "document" = the point i, "topic" = the coordinate c, draw index 0.
// random bits of (seed, global document index, stage [, topic], draw index)
TMVB_HD inline tmvb_philox4 tmvb_rng(uint64_t seed, uint64_t doc, uint32_t stage, uint32_t topic, uint32_t draw)
{
    return tmvb_philox4x32_10_raw((uint32_t)doc, (uint32_t)(doc >> 32), stage | (topic << 8), draw, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// 53-bit uniform in (0, 1): never 0, never 1 (log() of it is finite)
TMVB_HD inline double tmvb_u53_open(uint32_t hi, uint32_t lo)
{
    const uint64_t b = (((uint64_t)hi << 32) | lo) >> 12;                 // 52 bits
    return ((double)b + 0.5) * (1.0 / 4503599627370496.0);
}
// 53-bit uniform in [0, 1)
TMVB_HD inline double tmvb_u53(uint32_t hi, uint32_t lo)
{
    const uint64_t b = (((uint64_t)hi << 32) | lo) >> 11;                 // 53 bits
    return (double)b * (1.0 / 9007199254740992.0);
}
// 24-bit uniform in [0, 1), exact in fp32
TMVB_HD inline float tmvb_u24(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }
