// map_file.hpp -- the map on disk: the brick store's entries as one file (no reference counterpart: the reference's map dies with its process).
// Plain host C++ without HIP: the codec moves chunks of bricks through callbacks, so it runs -- and is tested -- without a GPU
// (tests/map_file_main.cpp, tests/test_map_file_abi_cpu.py).  HybKinectfu::saveMap / loadMap put kf_read_brick_store / kf_write_brick_store behind them.
//
// Format, version 1, little-endian, no padding:
//   offset   0  char[8]  magic "HYBKFMAP"
//            8  u32      version (1)
//           12  u32      resolution (voxels per axis)
//           16  u32      brick edge (8)
//           20  u32      colour flag (0 | 1)
//           24  u32      volume size in metres, the bits of the fp32
//           28  u32      max weight, the bits of the fp32
//           32  i32[3]   origin_vox: where the window stood (kf_volume_origin)
//           44  u32      frame_id: the last frame processed
//           48  f32[16]  the camera pose, row-major, in the window's coordinates at origin_vox
//          112  u64      n_bricks
//          120  u64      the store's `dropped` count at save time (non-zero: the map has holes)
//          128  n_bricks records: key i32[3] (world brick coordinate x, y, z), tsdf f32[512], weight f32[512] (true weights), then u8[1536] colour
//               if the flag is set -- kf_read_brick_store's layout; 4108 or 5644 bytes each
// Records are sorted by key (z, y, x) ascending, so the record section depends on the map alone, not on slot order or on where the window stands.
// The reader checks magic, version, brick edge, the file's length against the record size x n_bricks, and that the keys are in range, ascending
// and unique -- all before the caller is given anything to apply: a truncated or foreign file is refused, never half-loaded.
#pragma once
#include <stdint.h>
#include <functional>

#define HKF_MAP_VERSION 1u
#define HKF_MAP_HEADER_BYTES 128u
#define HKF_MAP_BRICK_VOX 512u

struct HkfMapHeader {
  uint32_t version, resolution, brick_edge, has_color;
  float size_m, max_weight;
  int32_t origin_vox[3];
  uint32_t frame_id;
  float pose[16];
  uint64_t n_bricks, dropped;
};

enum {
  HKF_MAP_OK = 0,
  HKF_MAP_ERR_IO = -1,         // cannot open, read, write or seek
  HKF_MAP_ERR_MAGIC = -2,      // shorter than a header, or not a map file
  HKF_MAP_ERR_VERSION = -3,
  HKF_MAP_ERR_BRICK = -4,      // brick edge other than 8, a colour flag other than 0 | 1
  HKF_MAP_ERR_LENGTH = -5,     // the file's length is not header + n_bricks records
  HKF_MAP_ERR_KEYS = -6,       // a key out of range, not ascending, or twice
  HKF_MAP_ERR_ARG = -7,
  HKF_MAP_ERR_CALLBACK = -8,   // a callback returned false (the source or the sink failed)
  HKF_MAP_ERR_REFUSED = -9     // the accept callback turned the header down: nothing was applied
};

static inline uint64_t hkf_map_record_bytes(bool color) { return 12u + 2u * HKF_MAP_BRICK_VOX * 4u + (color ? HKF_MAP_BRICK_VOX * 3u : 0u); }

// the source of a write: entries [first, first + count) in the source's own order; tsdf, weight and color may be NULL together (a pass over the keys only)
typedef std::function<bool(uint32_t first, uint32_t count, int32_t* keys, float* tsdf, float* weight, uint8_t* color)> HkfMapFetch;
// the sink of a read: the next `count` records, ascending by key; color is NULL without the flag
typedef std::function<bool(uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color)> HkfMapApply;
typedef std::function<bool(const HkfMapHeader&)> HkfMapAccept;

// Writes `path`: h.n_bricks entries fetched in chunks of at most `chunk` (>= 1) -- one pass over the keys, which fixes every record's place, then one
// pass over the bricks, each written at its place.  version and brick_edge are set here.  A key out of range or twice: HKF_MAP_ERR_KEYS.  On any error
// the file is removed.
int hkf_map_write(const char* path, const HkfMapHeader& h, uint32_t chunk, const HkfMapFetch& fetch);
// every check of the reader, and the header; nothing else is read into memory but the keys
int hkf_map_info(const char* path, HkfMapHeader* out);
// hkf_map_info's checks, then accept(header) (may be empty: accepted), then the records in chunks of at most `chunk`
int hkf_map_read(const char* path, uint32_t chunk, const HkfMapAccept& accept, const HkfMapApply& apply);

// Merging a map that was recorded in another world frame (HybKinectfu::mergeMap): the file's keys translated by a whole number of bricks.
// hkf_map_offset_keys: out[i] = keys[i] + offset (out may be keys itself; offset NULL: zero) for `count` keys of three components.  The sums are taken in
// 64 bits, so no int32 overflows, and every translated component must lie in the key range [-2^20, 2^20): false, with `out` untouched, when one does
// not.  Adding a constant keeps the (z, y, x) order of the records, so translated records need no re-sort.
bool hkf_map_offset_keys(uint32_t count, const int32_t* keys, const int32_t offset[3], int32_t* out);
// hkf_map_info's checks, then every key of the file translated by `offset`: HKF_MAP_ERR_KEYS when a translated key leaves the key range
int hkf_map_info_offset(const char* path, const int32_t offset[3], HkfMapHeader* out);
