// kf_tiff.h — native GeoTIFF window decode (kf_tiff.cpp), shared with the
// ingest ring (kf_stream.cpp) so granule bands decode straight into pinned slots.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace kf {
namespace tiff {
// rows [r0, r1) x columns [c0, c1) of sample `band` into dst (dense, row-major);
// elem_bytes > 0: throw unless the file's samples are exactly that size
void read_window(const std::string& path, int band, void* dst, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1,
                 int nthreads, int elem_bytes = 0);

// The chunks of sample `band` that intersect a window, for the device tile
// decoder (kf_inflate.hip): file offsets, byte counts and tile row / column
// (tile_rc[2 i], tile_rc[2 i + 1]), row-major, plus the layout facts that
// decide whether the device decoder can take the file.  A striped file has
// tile = 0 and an empty table.
struct TileTable {
  std::vector<uint64_t> offsets, counts;
  std::vector<int32_t> tile_rc;
  uint64_t width = 0, height = 0, tile = 0;
  int bits = 0, sample_format = 1, compression = 1, predictor = 1;
};
TileTable tile_table(const std::string& path, int band, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1);
// the byte ranges (offsets[i], counts[i]) of a file back to back into dst
void read_ranges(const std::string& path, const std::vector<uint64_t>& offsets, const std::vector<uint64_t>& counts,
                 void* dst, int nthreads);
}  // namespace tiff
}  // namespace kf
