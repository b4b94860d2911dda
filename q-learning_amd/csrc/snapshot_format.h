// Snapshot container and the host reference of the bitmap frame codec (host only: no HIP call, no HIP header).
//
// File (little-endian, no padding left unwritten, no time stamp):
//   FileHeader (64 B)  magic "QLXSNAP1", version, kind, n_sections, crc32c of header + table, file_bytes
//   SectionEntry x kMaxSections (32 B each; unused entries zero)  id, offset, bytes, checksum
//   sections, each at its entry's offset
// Small sections carry crc32c of their bytes.  Frame sections carry the 64-bit wrapping sum
//   sum over the 8-byte words w_j of the raw frames (j = frame ordinal * 882 + word) of w_j * ((2 j + 1) * kH1)
// (order-independent, every multiplier odd: any change of one word changes the sum).
//
// Frame section: FrameHeader {codec, chunk_frames C, n_frames, raw_bytes, stored_bytes}, then stored_bytes of payload:
//   QLX_FRAME_CODEC_RAW     n_frames x 7,056 bytes
//   QLX_FRAME_CODEC_BITMAP  chunks of up to C frames, in frame order, each
//       {u32 n_frames, u32 value_bytes}, u16 nnz[n_frames] zero-padded to 8 bytes, masks [n_frames][882],
//       values [value_bytes] = the non-zero bytes of the frames in frame order, ascending byte index
//     mask bit (i & 7) of byte (i >> 3) is set iff byte i of the frame is non-zero.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/qlx.h"

namespace qlx {
namespace snap {

struct FormatError {   // the callers turn it into QLX_E_IO
  std::string msg;
};

constexpr uint32_t kFrameBytes = 7056, kMaskBytes = 882, kFrameWords = 882;
constexpr uint32_t kChunkFrames = 512;   // C of the files this build writes (a reader takes the section's own)
constexpr uint32_t kMaxChunkFrames = 4096;
constexpr uint32_t kMaxSections = 16;
constexpr uint64_t kChecksumMul = 0x9E3779B97F4A7C15ull;   // kH1 of the env checksum

enum SectionId : uint32_t {
  SEC_INFO = 1, SEC_LEARNER = 2, SEC_ENV = 3, SEC_ENV_FRAMES = 4, SEC_REPLAY = 5, SEC_REPLAY_FRAMES = 6,
  SEC_MODEL_ONLINE = 7, SEC_MODEL_TARGET = 8, SEC_BOOKS = 9, SEC_PER = 10, SEC_MEMO = 11
};

struct FileHeader {
  char magic[8];
  uint32_t version, kind, n_sections, crc;
  uint64_t file_bytes;
  uint8_t zero[32];
};
struct SectionEntry {
  uint32_t id, zero;
  uint64_t offset, bytes, checksum;
};
struct FrameHeader {
  uint32_t codec, chunk_frames;
  uint64_t n_frames, raw_bytes, stored_bytes;
};
struct ChunkHeader {
  uint32_t n_frames, value_bytes;
};
static_assert(sizeof(FileHeader) == 64 && sizeof(SectionEntry) == 32 && sizeof(FrameHeader) == 32 && sizeof(ChunkHeader) == 8,
              "snapshot container layout");
constexpr uint64_t kDataStart = sizeof(FileHeader) + kMaxSections * sizeof(SectionEntry);

// ---- bitmap codec, host reference ----
// bytes of a chunk before its values: header, nnz table, masks
inline uint64_t chunk_fixed_bytes(uint32_t n) { return 8 + ((2ull * n + 7) & ~7ull) + (uint64_t)kMaskBytes * n; }
inline uint64_t chunk_mask_offset(uint32_t n) { return 8 + ((2ull * n + 7) & ~7ull); }
// worst case (every byte non-zero): 7,938 B per frame + the header and padding
inline uint64_t chunk_max_bytes(uint32_t n) { return chunk_fixed_bytes(n) + (uint64_t)kFrameBytes * n; }
// frames [n][7056] -> out (room for chunk_max_bytes(n)); returns the chunk's bytes
uint64_t pack_chunk(const uint8_t* frames, uint32_t n, uint8_t* out);
// everything a kernel's addressing depends on: n_frames in 1..max_frames, the chunk's size, every nnz <= 7056 and equal
// to its mask's popcount, the nnz sum equal to value_bytes, zero padding.  Throws FormatError naming what is wrong.
void validate_chunk(const uint8_t* buf, uint64_t bytes, uint32_t max_frames);
// a validated chunk -> frames [n][7056]
void unpack_chunk(const uint8_t* buf, uint8_t* frames);
// the frame checksum of n frames whose first has ordinal `first` in its section
uint64_t frame_checksum(const uint8_t* frames, uint64_t n, uint64_t first);

// ---- small sections: fixed-width fields appended / read back in order ----
struct Blob {
  std::vector<uint8_t> bytes;
  void put(const void* p, uint64_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    bytes.insert(bytes.end(), b, b + n);
  }
  void u32(uint32_t v) { put(&v, 4); }
  void u64(uint64_t v) { put(&v, 8); }
  void f32(float v) { put(&v, 4); }
  uint8_t* grow(uint64_t n) {   // n zero bytes at the end, to be filled by the caller
    bytes.resize(bytes.size() + n, 0);
    return bytes.data() + bytes.size() - n;
  }
};
class BlobReader {   // every read is bounds-checked; done() requires that nothing is left
 public:
  BlobReader(const std::vector<uint8_t>& b, uint32_t id) : b_(b), id_(id) {}
  const uint8_t* take(uint64_t n) {
    if (n > b_.size() - at_) throw FormatError{"snapshot: section " + std::to_string(id_) + " is shorter than its fields"};
    at_ += n;
    return b_.data() + at_ - n;
  }
  void get(void* out, uint64_t n) { const uint8_t* p = take(n); for (uint64_t i = 0; i < n; ++i) static_cast<uint8_t*>(out)[i] = p[i]; }
  uint32_t u32() { uint32_t v; get(&v, 4); return v; }
  uint64_t u64() { uint64_t v; get(&v, 8); return v; }
  float f32() { float v; get(&v, 4); return v; }
  void done() const {
    if (at_ != b_.size()) throw FormatError{"snapshot: section " + std::to_string(id_) + " is longer than its fields"};
  }

 private:
  const std::vector<uint8_t>& b_;
  uint32_t id_;
  uint64_t at_ = 0;
};

// ---- container ----
class Writer {   // writes path + ".tmp"; finish() flushes and renames it over path; otherwise the destructor removes it
 public:
  Writer(const std::string& path, uint32_t kind);
  ~Writer();
  Writer(const Writer&) = delete;
  Writer& operator=(const Writer&) = delete;
  void small(uint32_t id, const void* data, uint64_t bytes);   // a whole section with its crc32c
  void begin(uint32_t id);
  void append(const void* data, uint64_t bytes);
  void rewrite(uint64_t section_offset, const void* data, uint64_t bytes);   // inside the open section
  void end(uint64_t checksum);
  uint64_t position() const { return pos_; }   // file offset of the next byte
  uint64_t finish();                            // returns the file's size

 private:
  void put(const void* data, uint64_t bytes);
  std::string path_, tmp_;
  FILE* f_ = nullptr;
  uint32_t kind_;
  uint64_t pos_ = 0;
  std::vector<SectionEntry> table_;
  bool open_ = false;
};

class Reader {   // validates magic, version, kind (0 = any), size, the table's crc and every section's range on open
 public:
  Reader(const std::string& path, uint32_t kind);
  ~Reader();
  Reader(const Reader&) = delete;
  Reader& operator=(const Reader&) = delete;
  const FileHeader& header() const { return hdr_; }
  const SectionEntry* find(uint32_t id) const;
  const SectionEntry& need(uint32_t id) const;
  std::vector<uint8_t> small(uint32_t id, uint64_t max_bytes = 1ull << 32);   // reads the section, checks its crc32c
  void seek(uint64_t offset);
  void read(void* out, uint64_t bytes);

 private:
  std::string path_;
  FILE* f_ = nullptr;
  FileHeader hdr_{};
  std::vector<SectionEntry> table_;
};

// Frame sections chunk by chunk; the device pipeline (frame_codec.hip) and the host helpers below share these.
class FrameSectionWriter {
 public:
  FrameSectionWriter(Writer& w, uint32_t id, uint32_t codec, uint32_t chunk_frames, uint64_t n_frames);
  void append(const void* data, uint64_t bytes) { w_.append(data, bytes); stored_ += bytes; }
  void end(uint64_t checksum);
  uint64_t stored() const { return stored_; }

 private:
  Writer& w_;
  FrameHeader h_{};
  uint64_t stored_ = 0;
};

class FrameSectionReader {
 public:
  FrameSectionReader(Reader& r, uint32_t id, uint64_t expect_frames);
  const FrameHeader& header() const { return h_; }
  uint64_t checksum() const { return checksum_; }
  uint64_t frames_left() const { return h_.n_frames - done_; }
  // bitmap: the next chunk, validated, into buf (room for chunk_max_bytes(header().chunk_frames)); its frame count
  uint32_t next_chunk(uint8_t* buf, uint64_t* bytes);
  // raw: the next n frames into buf
  void next_raw(uint8_t* buf, uint32_t n);
  void finish();   // every frame and every byte of the section consumed

 private:
  Reader& r_;
  FrameHeader h_{};
  uint64_t checksum_ = 0, left_ = 0, done_ = 0;
};

// whole frame sections through the host reference (tests of the container; the library packs on the device)
void write_frames_host(Writer& w, uint32_t id, const uint8_t* frames, uint64_t n, uint32_t codec, uint32_t chunk_frames);
void read_frames_host(Reader& r, uint32_t id, uint64_t n, uint8_t* frames);

// qlx_snapshot_info of a file: header + SEC_INFO only
void read_info(const std::string& path, qlx_snapshot_info* out);

}  // namespace snap
}  // namespace qlx
