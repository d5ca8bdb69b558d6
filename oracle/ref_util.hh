// ORACLE / TEST INFRASTRUCTURE ONLY -- never shipped, never measured.
//
// What the golden-vector generators share (ref_fixed.cc, ref_var.cc): hex and
// JSON quoting, sha256 for the streams too long to store, and the seeded
// generator of the field values.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ref_util {
using std::string;
using std::vector;

inline string hex(const void *p, size_t n) {
  static const char *d = "0123456789abcdef";
  string s;
  const uint8_t *b = static_cast<const uint8_t *>(p);
  for (size_t i = 0; i < n; ++i) { s += d[b[i] >> 4]; s += d[b[i] & 15]; }
  return s;
}
inline string q(const string &s) { return "\"" + s + "\""; }

// ---- sha256 (FIPS 180-4)
inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
inline string sha256(const uint8_t *msg, size_t len) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                   0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  vector<uint8_t> m(msg, msg + len);
  m.push_back(0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  for (int i = 7; i >= 0; --i) m.push_back(uint8_t((uint64_t(len) * 8) >> (8 * i)));
  for (size_t b = 0; b < m.size(); b += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(m[b + 4 * i]) << 24 | uint32_t(m[b + 4 * i + 1]) << 16 |
             uint32_t(m[b + 4 * i + 2]) << 8 | m[b + 4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a[8];
    memcpy(a, h, sizeof a);
    for (int i = 0; i < 64; ++i) {
      const uint32_t S1 = rotr(a[4], 6) ^ rotr(a[4], 11) ^ rotr(a[4], 25);
      const uint32_t ch = (a[4] & a[5]) ^ (~a[4] & a[6]);
      const uint32_t t1 = a[7] + S1 + ch + K[i] + w[i];
      const uint32_t S0 = rotr(a[0], 2) ^ rotr(a[0], 13) ^ rotr(a[0], 22);
      const uint32_t mj = (a[0] & a[1]) ^ (a[0] & a[2]) ^ (a[1] & a[2]);
      const uint32_t t2 = S0 + mj;
      for (int k = 7; k > 0; --k) a[k] = a[k - 1];
      a[4] += t1;
      a[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) h[i] += a[i];
  }
  uint8_t out[32];
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 4; ++k) out[4 * i + k] = uint8_t(h[i] >> (24 - 8 * k));
  return hex(out, 32);
}

// ---- the generator
struct rng {
  uint64_t s;
  uint64_t operator()() {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};

}  // namespace ref_util
