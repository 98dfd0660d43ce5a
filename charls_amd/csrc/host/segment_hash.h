// segment_hash.h -- the body of jls::segment_hash (seek_index.h), in a header of its own so that the CPU harness of the device
// kernel (device/segment_hash.hip, tests/emu/emu_hash_driver.cpp) compares against this very function.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace jls {

inline uint64_t segment_hash_bytes(const uint8_t* p, size_t n) noexcept
{
    // A multiply-rotate round per 8 bytes (the shape of xxHash64's round) and murmur3's finaliser.
    constexpr uint64_t k1 = 0x9E3779B185EBCA87ull, k2 = 0xC2B2AE3D27D4EB4Full;
    uint64_t h = 0x27D4EB2F165667C5ull ^ (static_cast<uint64_t>(n) * k1);
    size_t i = 0;
    for (; i + 8 <= n; i += 8)
    {
        uint64_t w;
        std::memcpy(&w, p + i, sizeof w); // (the library runs on little-endian hosts only, as the device does)
        w *= k2;
        w = (w << 31) | (w >> 33);
        h ^= w * k1;
        h = ((h << 27) | (h >> 37)) * k1 + 0x85EBCA77C2B2AE63ull;
    }
    uint64_t tail = 0;
    if (i < n)
        std::memcpy(&tail, p + i, n - i);
    h ^= tail * k2;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

} // namespace jls
