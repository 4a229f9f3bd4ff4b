// map_file.cpp -- the codec of map_file.hpp: plain host C++, no HIP, no device.
#include "map_file.hpp"
#include "../csrc/brick_key.h"
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>

static const char kMagic[8] = {'H', 'Y', 'B', 'K', 'F', 'M', 'A', 'P'};

// the fields at their offsets, byte by byte: the file is little-endian whatever the host is
static void put32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
static void put64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
static uint32_t get32(const uint8_t* p) { uint32_t v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)p[i] << (8 * i); return v; }
static uint64_t get64(const uint8_t* p) { uint64_t v = 0; for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i); return v; }
static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static void encode_header(const HkfMapHeader& h, uint8_t out[HKF_MAP_HEADER_BYTES]) {
  memcpy(out, kMagic, 8);
  put32(out + 8, HKF_MAP_VERSION); put32(out + 12, h.resolution); put32(out + 16, 8u); put32(out + 20, h.has_color ? 1u : 0u);
  put32(out + 24, f2u(h.size_m)); put32(out + 28, f2u(h.max_weight));
  for (int k = 0; k < 3; ++k) put32(out + 32 + 4 * k, (uint32_t)h.origin_vox[k]);
  put32(out + 44, h.frame_id);
  for (int k = 0; k < 16; ++k) put32(out + 48 + 4 * k, f2u(h.pose[k]));
  put64(out + 112, h.n_bricks); put64(out + 120, h.dropped);
}
static void decode_header(const uint8_t in[HKF_MAP_HEADER_BYTES], HkfMapHeader& h) {
  h.version = get32(in + 8); h.resolution = get32(in + 12); h.brick_edge = get32(in + 16); h.has_color = get32(in + 20);
  h.size_m = u2f(get32(in + 24)); h.max_weight = u2f(get32(in + 28));
  for (int k = 0; k < 3; ++k) h.origin_vox[k] = (int32_t)get32(in + 32 + 4 * k);
  h.frame_id = get32(in + 44);
  for (int k = 0; k < 16; ++k) h.pose[k] = u2f(get32(in + 48 + 4 * k));
  h.n_bricks = get64(in + 112); h.dropped = get64(in + 120);
}

// the order of the records: (z, y, x) ascending as signed numbers -- each component biased into 21 unsigned bits, z on top
static bool key_in_range(const int32_t k[3]) { return kf_brick_key_in_range(k[0]) && kf_brick_key_in_range(k[1]) && kf_brick_key_in_range(k[2]); }
static uint64_t order_word(const int32_t k[3]) {
  const int64_t bias = -(int64_t)KF_BRICK_KEY_MIN;
  return ((uint64_t)(k[2] + bias) << (2 * KF_BRICK_KEY_BITS)) | ((uint64_t)(k[1] + bias) << KF_BRICK_KEY_BITS) | (uint64_t)(k[0] + bias);
}

// host arrays <-> the record's little-endian words (a plain copy on a little-endian host)
static void words_out(uint8_t* dst, const void* src, size_t n_words) {
  const uint8_t* s = (const uint8_t*)src;
  for (size_t i = 0; i < n_words; ++i) { uint32_t v; memcpy(&v, s + 4 * i, 4); put32(dst + 4 * i, v); }
}
static void words_in(void* dst, const uint8_t* src, size_t n_words) {
  uint8_t* d = (uint8_t*)dst;
  for (size_t i = 0; i < n_words; ++i) { const uint32_t v = get32(src + 4 * i); memcpy(d + 4 * i, &v, 4); }
}

static bool seek_to(FILE* f, uint64_t off) { return fseeko(f, (off_t)off, SEEK_SET) == 0; }   // (64-bit offsets: a map may exceed 2 GiB)

int hkf_map_write(const char* path, const HkfMapHeader& h, uint32_t chunk, const HkfMapFetch& fetch) {
  if (!path || !fetch || chunk == 0 || h.n_bricks > 0xFFFFFFFFull) return HKF_MAP_ERR_ARG;
  const uint32_t n = (uint32_t)h.n_bricks;
  const bool color = h.has_color != 0;
  const uint64_t rec = hkf_map_record_bytes(color);
  // pass 1, keys only: rank[i] = the place of source entry i among the records
  std::vector<int32_t> keys((size_t)n * 3);
  for (uint32_t first = 0; first < n; first += chunk) {
    const uint32_t c = n - first < chunk ? n - first : chunk;
    if (!fetch(first, c, keys.data() + 3 * (size_t)first, nullptr, nullptr, nullptr)) return HKF_MAP_ERR_CALLBACK;
  }
  std::vector<uint64_t> word(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (!key_in_range(&keys[3 * (size_t)i])) return HKF_MAP_ERR_KEYS;
    word[i] = order_word(&keys[3 * (size_t)i]);
  }
  std::vector<uint32_t> by_key(n), rank(n);
  std::iota(by_key.begin(), by_key.end(), 0u);
  std::sort(by_key.begin(), by_key.end(), [&](uint32_t a, uint32_t b) { return word[a] < word[b]; });
  for (uint32_t r = 0; r < n; ++r) {
    if (r && word[by_key[r]] == word[by_key[r - 1]]) return HKF_MAP_ERR_KEYS;
    rank[by_key[r]] = r;
  }
  FILE* f = fopen(path, "wb");
  if (!f) return HKF_MAP_ERR_IO;
  int st = HKF_MAP_OK;
  uint8_t head[HKF_MAP_HEADER_BYTES];
  encode_header(h, head);
  if (fwrite(head, 1, sizeof(head), f) != sizeof(head)) st = HKF_MAP_ERR_IO;
  // pass 2: the bricks, each record at its place
  const uint32_t cap = n < chunk ? n : chunk;
  std::vector<int32_t> ck((size_t)cap * 3);
  std::vector<float> ct((size_t)cap * HKF_MAP_BRICK_VOX), cw((size_t)cap * HKF_MAP_BRICK_VOX);
  std::vector<uint8_t> cc(color ? (size_t)cap * HKF_MAP_BRICK_VOX * 3 : 0), out((size_t)rec);
  for (uint32_t first = 0; first < n && st == HKF_MAP_OK; first += chunk) {
    const uint32_t c = n - first < chunk ? n - first : chunk;
    if (!fetch(first, c, ck.data(), ct.data(), cw.data(), color ? cc.data() : nullptr)) { st = HKF_MAP_ERR_CALLBACK; break; }
    for (uint32_t i = 0; i < c && st == HKF_MAP_OK; ++i) {
      if (memcmp(&ck[3 * (size_t)i], &keys[3 * (size_t)(first + i)], 12) != 0) { st = HKF_MAP_ERR_CALLBACK; break; }   // the source changed between the passes
      words_out(out.data(), &ck[3 * (size_t)i], 3);
      words_out(out.data() + 12, &ct[(size_t)i * HKF_MAP_BRICK_VOX], HKF_MAP_BRICK_VOX);
      words_out(out.data() + 12 + 4 * HKF_MAP_BRICK_VOX, &cw[(size_t)i * HKF_MAP_BRICK_VOX], HKF_MAP_BRICK_VOX);
      if (color) memcpy(out.data() + 12 + 8 * HKF_MAP_BRICK_VOX, &cc[(size_t)i * HKF_MAP_BRICK_VOX * 3], HKF_MAP_BRICK_VOX * 3);
      if (!seek_to(f, HKF_MAP_HEADER_BYTES + rec * rank[first + i]) || fwrite(out.data(), 1, out.size(), f) != out.size()) st = HKF_MAP_ERR_IO;
    }
  }
  if (fclose(f) != 0 && st == HKF_MAP_OK) st = HKF_MAP_ERR_IO;
  if (st != HKF_MAP_OK) remove(path);
  return st;
}

bool hkf_map_offset_keys(uint32_t count, const int32_t* keys, const int32_t offset[3], int32_t* out) {
  if (count && (!keys || !out)) return false;
  for (int pass = 0; pass < 2; ++pass) {                       // all checked before the first is written
    for (size_t i = 0; i < (size_t)count * 3; ++i) {
      const int64_t t = (int64_t)keys[i] + (offset ? offset[i % 3] : 0);
      if (pass == 0) { if (!kf_brick_key_in_range(t)) return false; }
      else out[i] = (int32_t)t;
    }
  }
  return true;
}

// every check; leaves `f` anywhere.  offset != nullptr: every key must stay in range when translated by it
static int check_file(FILE* f, HkfMapHeader& h, const int32_t* offset = nullptr) {
  uint8_t head[HKF_MAP_HEADER_BYTES];
  if (!seek_to(f, 0)) return HKF_MAP_ERR_IO;
  if (fread(head, 1, sizeof(head), f) != sizeof(head) || memcmp(head, kMagic, 8) != 0) return HKF_MAP_ERR_MAGIC;
  decode_header(head, h);
  if (h.version != HKF_MAP_VERSION) return HKF_MAP_ERR_VERSION;
  if (h.brick_edge != 8u || h.has_color > 1u) return HKF_MAP_ERR_BRICK;
  const uint64_t rec = hkf_map_record_bytes(h.has_color != 0);
  if (h.n_bricks > 0xFFFFFFFFull) return HKF_MAP_ERR_LENGTH;
  if (fseeko(f, 0, SEEK_END) != 0) return HKF_MAP_ERR_IO;
  const long long len = (long long)ftello(f);
  if (len < 0) return HKF_MAP_ERR_IO;
  if ((uint64_t)len != HKF_MAP_HEADER_BYTES + rec * h.n_bricks) return HKF_MAP_ERR_LENGTH;
  uint64_t last = 0;
  for (uint64_t i = 0; i < h.n_bricks; ++i) {
    uint8_t kb[12]; int32_t k[3];
    if (!seek_to(f, HKF_MAP_HEADER_BYTES + rec * i) || fread(kb, 1, 12, f) != 12) return HKF_MAP_ERR_IO;
    words_in(k, kb, 3);
    if (!key_in_range(k)) return HKF_MAP_ERR_KEYS;
    const uint64_t w = order_word(k);
    if (i && w <= last) return HKF_MAP_ERR_KEYS;
    last = w;
    if (offset && !hkf_map_offset_keys(1, k, offset, k)) return HKF_MAP_ERR_KEYS;
  }
  return HKF_MAP_OK;
}

int hkf_map_info_offset(const char* path, const int32_t offset[3], HkfMapHeader* out) {
  if (!path || !out) return HKF_MAP_ERR_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return HKF_MAP_ERR_IO;
  HkfMapHeader h;
  memset(&h, 0, sizeof(h));
  const int st = check_file(f, h, offset);
  fclose(f);
  if (st == HKF_MAP_OK) *out = h;
  return st;
}
int hkf_map_info(const char* path, HkfMapHeader* out) { return hkf_map_info_offset(path, nullptr, out); }

int hkf_map_read(const char* path, uint32_t chunk, const HkfMapAccept& accept, const HkfMapApply& apply) {
  if (!path || !apply || chunk == 0) return HKF_MAP_ERR_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return HKF_MAP_ERR_IO;
  HkfMapHeader h;
  memset(&h, 0, sizeof(h));
  int st = check_file(f, h);
  if (st == HKF_MAP_OK && accept && !accept(h)) st = HKF_MAP_ERR_REFUSED;
  if (st == HKF_MAP_OK && !seek_to(f, HKF_MAP_HEADER_BYTES)) st = HKF_MAP_ERR_IO;
  if (st == HKF_MAP_OK) {
    const bool color = h.has_color != 0;
    const uint64_t rec = hkf_map_record_bytes(color);
    const uint32_t n = (uint32_t)h.n_bricks, cap = n < chunk ? n : chunk;
    std::vector<int32_t> ck((size_t)cap * 3);
    std::vector<float> ct((size_t)cap * HKF_MAP_BRICK_VOX), cw((size_t)cap * HKF_MAP_BRICK_VOX);
    std::vector<uint8_t> cc(color ? (size_t)cap * HKF_MAP_BRICK_VOX * 3 : 0), in((size_t)rec);
    for (uint32_t first = 0; first < n && st == HKF_MAP_OK; first += chunk) {
      const uint32_t c = n - first < chunk ? n - first : chunk;
      for (uint32_t i = 0; i < c; ++i) {
        if (fread(in.data(), 1, in.size(), f) != in.size()) { st = HKF_MAP_ERR_IO; break; }
        words_in(&ck[3 * (size_t)i], in.data(), 3);
        words_in(&ct[(size_t)i * HKF_MAP_BRICK_VOX], in.data() + 12, HKF_MAP_BRICK_VOX);
        words_in(&cw[(size_t)i * HKF_MAP_BRICK_VOX], in.data() + 12 + 4 * HKF_MAP_BRICK_VOX, HKF_MAP_BRICK_VOX);
        if (color) memcpy(&cc[(size_t)i * HKF_MAP_BRICK_VOX * 3], in.data() + 12 + 8 * HKF_MAP_BRICK_VOX, HKF_MAP_BRICK_VOX * 3);
      }
      if (st == HKF_MAP_OK && !apply(c, ck.data(), ct.data(), cw.data(), color ? cc.data() : nullptr)) st = HKF_MAP_ERR_CALLBACK;
    }
  }
  fclose(f);
  return st;
}
