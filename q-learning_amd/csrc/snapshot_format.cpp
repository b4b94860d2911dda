// Snapshot container and the host reference of the bitmap frame codec (snapshot_format.h).  Host code only.
#include "snapshot_format.h"

#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "crc32c.h"

namespace qlx {
namespace snap {

namespace {

const char kMagic[8] = {'Q', 'L', 'X', 'S', 'N', 'A', 'P', '1'};

[[noreturn]] void fail(const std::string& msg) { throw FormatError{"snapshot: " + msg}; }

uint32_t header_crc(FileHeader h, const SectionEntry* table) {
  h.crc = 0;
  std::vector<uint8_t> buf(kDataStart);
  std::memcpy(buf.data(), &h, sizeof(h));
  std::memcpy(buf.data() + sizeof(h), table, kMaxSections * sizeof(SectionEntry));
  return crc32c(buf.data(), buf.size());
}

inline uint32_t load_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

}  // namespace

// ---- codec ----
uint64_t pack_chunk(const uint8_t* frames, uint32_t n, uint8_t* out) {
  const uint64_t mask_off = chunk_mask_offset(n), fixed = chunk_fixed_bytes(n);
  std::memset(out, 0, fixed);
  uint8_t* values = out + fixed;
  uint64_t vb = 0;
  for (uint32_t f = 0; f < n; ++f) {
    const uint8_t* src = frames + (uint64_t)f * kFrameBytes;
    uint8_t* mask = out + mask_off + (uint64_t)f * kMaskBytes;
    uint32_t nnz = 0;
    for (uint32_t i = 0; i < kFrameBytes; ++i) {
      if (!src[i]) continue;
      mask[i >> 3] |= (uint8_t)(1u << (i & 7));
      values[vb + nnz++] = src[i];
    }
    out[8 + 2 * f] = (uint8_t)nnz;
    out[8 + 2 * f + 1] = (uint8_t)(nnz >> 8);
    vb += nnz;
  }
  const ChunkHeader h{n, (uint32_t)vb};
  std::memcpy(out, &h, sizeof(h));
  return fixed + vb;
}

void validate_chunk(const uint8_t* buf, uint64_t bytes, uint32_t max_frames) {
  if (bytes < sizeof(ChunkHeader)) fail("frame chunk shorter than its header");
  ChunkHeader h;
  std::memcpy(&h, buf, sizeof(h));
  if (h.n_frames == 0 || h.n_frames > max_frames)
    fail("frame chunk n_frames " + std::to_string(h.n_frames) + " outside 1.." + std::to_string(max_frames));
  const uint64_t fixed = chunk_fixed_bytes(h.n_frames);
  if (bytes != fixed + h.value_bytes) fail("frame chunk size disagrees with its n_frames / value_bytes");
  const uint64_t mask_off = chunk_mask_offset(h.n_frames);
  for (uint64_t i = 8 + 2ull * h.n_frames; i < mask_off; ++i)
    if (buf[i]) fail("frame chunk nnz padding is not zero");
  uint64_t sum = 0;
  for (uint32_t f = 0; f < h.n_frames; ++f) {
    const uint32_t nnz = load_u16(buf + 8 + 2 * f);
    if (nnz > kFrameBytes) fail("frame chunk nnz above the frame size");
    const uint8_t* mask = buf + mask_off + (uint64_t)f * kMaskBytes;
    uint32_t pop = 0;
    uint32_t i = 0;
    for (; i + 8 <= kMaskBytes; i += 8) {
      uint64_t w;
      std::memcpy(&w, mask + i, 8);
      pop += (uint32_t)__builtin_popcountll(w);
    }
    for (; i < kMaskBytes; ++i) pop += (uint32_t)__builtin_popcount(mask[i]);
    if (pop != nnz) fail("frame chunk nnz disagrees with its mask (frame " + std::to_string(f) + ")");
    sum += nnz;
  }
  if (sum != h.value_bytes) fail("frame chunk nnz sum disagrees with value_bytes");
}

void unpack_chunk(const uint8_t* buf, uint8_t* frames) {
  ChunkHeader h;
  std::memcpy(&h, buf, sizeof(h));
  const uint64_t mask_off = chunk_mask_offset(h.n_frames);
  const uint8_t* values = buf + chunk_fixed_bytes(h.n_frames);
  uint64_t v = 0;
  for (uint32_t f = 0; f < h.n_frames; ++f) {
    const uint8_t* mask = buf + mask_off + (uint64_t)f * kMaskBytes;
    uint8_t* dst = frames + (uint64_t)f * kFrameBytes;
    for (uint32_t i = 0; i < kFrameBytes; ++i) dst[i] = (mask[i >> 3] >> (i & 7)) & 1 ? values[v++] : 0;
  }
}

uint64_t frame_checksum(const uint8_t* frames, uint64_t n, uint64_t first) {
  uint64_t sum = 0;
  for (uint64_t f = 0; f < n; ++f)
    for (uint32_t k = 0; k < kFrameWords; ++k) {
      uint64_t w;
      std::memcpy(&w, frames + f * kFrameBytes + 8ull * k, 8);
      const uint64_t j = (first + f) * kFrameWords + k;
      sum += w * ((2 * j + 1) * kChecksumMul);
    }
  return sum;
}

// ---- writer ----
Writer::Writer(const std::string& path, uint32_t kind) : path_(path), tmp_(path + ".tmp"), kind_(kind) {
  f_ = std::fopen(tmp_.c_str(), "wb");
  if (!f_) fail("cannot open " + tmp_ + " for writing");
  const std::vector<uint8_t> zeros(kDataStart, 0);   // the header and table are written by finish()
  put(zeros.data(), zeros.size());
}

Writer::~Writer() {
  if (f_) {
    std::fclose(f_);
    std::remove(tmp_.c_str());
  }
}

void Writer::put(const void* data, uint64_t bytes) {
  if (bytes && std::fwrite(data, 1, bytes, f_) != bytes) fail("write to " + tmp_ + " failed");
  pos_ += bytes;
}

void Writer::begin(uint32_t id) {
  if (open_ || table_.size() >= kMaxSections) fail("writer: section order");
  table_.push_back(SectionEntry{id, 0, pos_, 0, 0});
  open_ = true;
}

void Writer::append(const void* data, uint64_t bytes) {
  if (!open_) fail("writer: no open section");
  put(data, bytes);
}

void Writer::rewrite(uint64_t section_offset, const void* data, uint64_t bytes) {
  if (!open_ || table_.back().offset + section_offset + bytes > pos_) fail("writer: rewrite outside the open section");
  if (std::fseek(f_, (long)(table_.back().offset + section_offset), SEEK_SET) != 0 || std::fwrite(data, 1, bytes, f_) != bytes ||
      std::fseek(f_, (long)pos_, SEEK_SET) != 0)
    fail("write to " + tmp_ + " failed");
}

void Writer::end(uint64_t checksum) {
  if (!open_) fail("writer: no open section");
  table_.back().bytes = pos_ - table_.back().offset;
  table_.back().checksum = checksum;
  open_ = false;
}

void Writer::small(uint32_t id, const void* data, uint64_t bytes) {
  begin(id);
  append(data, bytes);
  end(crc32c(static_cast<const uint8_t*>(data), bytes));
}

uint64_t Writer::finish() {
  if (open_) fail("writer: a section is still open");
  FileHeader h{};
  std::memcpy(h.magic, kMagic, 8);
  h.version = QLX_SNAPSHOT_VERSION;
  h.kind = kind_;
  h.n_sections = (uint32_t)table_.size();
  h.file_bytes = pos_;
  SectionEntry table[kMaxSections] = {};
  std::copy(table_.begin(), table_.end(), table);
  h.crc = header_crc(h, table);
  bool ok = std::fseek(f_, 0, SEEK_SET) == 0 && std::fwrite(&h, sizeof(h), 1, f_) == 1 &&
            std::fwrite(table, sizeof(SectionEntry), kMaxSections, f_) == kMaxSections && std::fflush(f_) == 0 &&
            ::fsync(fileno(f_)) == 0;
  ok = (std::fclose(f_) == 0) && ok;
  f_ = nullptr;
  if (!ok || std::rename(tmp_.c_str(), path_.c_str()) != 0) {
    std::remove(tmp_.c_str());
    fail("writing " + path_ + " failed");
  }
  return pos_;
}

// ---- reader ----
Reader::Reader(const std::string& path, uint32_t kind) : path_(path) {
  f_ = std::fopen(path.c_str(), "rb");
  if (!f_) fail("cannot open " + path);
  try {
    if (std::fseek(f_, 0, SEEK_END) != 0) fail("cannot seek in " + path);
    const long size = std::ftell(f_);
    std::rewind(f_);
    if (size < (long)sizeof(FileHeader)) fail(path + " is shorter than a snapshot header (short file)");
    if (std::fread(&hdr_, sizeof(hdr_), 1, f_) != 1) fail("cannot read the header of " + path);
    if (std::memcmp(hdr_.magic, kMagic, 8) != 0) fail(path + " has a bad magic (not a qlx snapshot)");
    if (hdr_.version != QLX_SNAPSHOT_VERSION)
      fail("format version " + std::to_string(hdr_.version) + " of " + path + ", this build reads version " +
           std::to_string(QLX_SNAPSHOT_VERSION));
    if ((uint64_t)size < kDataStart) fail(path + " ends inside its section table (short file)");
    SectionEntry table[kMaxSections];
    if (std::fread(table, sizeof(SectionEntry), kMaxSections, f_) != kMaxSections) fail("cannot read the section table of " + path);
    if (header_crc(hdr_, table) != hdr_.crc) fail("header checksum mismatch in " + path);
    if (hdr_.file_bytes != (uint64_t)size)
      fail(path + " holds " + std::to_string(size) + " bytes, its header says " + std::to_string(hdr_.file_bytes) + " (short file)");
    if (hdr_.n_sections > kMaxSections) fail("too many sections in " + path);
    if (kind != 0 && hdr_.kind != kind)
      fail("wrong kind " + std::to_string(hdr_.kind) + " in " + path + ", expected " + std::to_string(kind));
    table_.assign(table, table + hdr_.n_sections);
    for (const SectionEntry& e : table_)
      if (e.offset < kDataStart || e.offset > hdr_.file_bytes || e.bytes > hdr_.file_bytes - e.offset)
        fail("section " + std::to_string(e.id) + " reaches past the end of " + path);
  } catch (...) {
    std::fclose(f_);
    f_ = nullptr;
    throw;
  }
}

Reader::~Reader() {
  if (f_) std::fclose(f_);
}

const SectionEntry* Reader::find(uint32_t id) const {
  for (const SectionEntry& e : table_)
    if (e.id == id) return &e;
  return nullptr;
}

const SectionEntry& Reader::need(uint32_t id) const {
  const SectionEntry* e = find(id);
  if (!e) fail("section " + std::to_string(id) + " is missing in " + path_);
  return *e;
}

void Reader::seek(uint64_t offset) {
  if (std::fseek(f_, (long)offset, SEEK_SET) != 0) fail("cannot seek in " + path_);
}

void Reader::read(void* out, uint64_t bytes) {
  if (bytes && std::fread(out, 1, bytes, f_) != bytes) fail("short read from " + path_);
}

std::vector<uint8_t> Reader::small(uint32_t id, uint64_t max_bytes) {
  const SectionEntry& e = need(id);
  if (e.bytes > max_bytes) fail("section " + std::to_string(id) + " is larger than it can be");
  std::vector<uint8_t> buf(e.bytes);
  seek(e.offset);
  read(buf.data(), buf.size());
  if (crc32c(buf.data(), buf.size()) != e.checksum) fail("checksum mismatch in section " + std::to_string(id) + " of " + path_);
  return buf;
}

// ---- frame sections ----
FrameSectionWriter::FrameSectionWriter(Writer& w, uint32_t id, uint32_t codec, uint32_t chunk_frames, uint64_t n_frames) : w_(w) {
  h_.codec = codec;
  h_.chunk_frames = chunk_frames;
  h_.n_frames = n_frames;
  h_.raw_bytes = n_frames * kFrameBytes;
  w_.begin(id);
  w_.append(&h_, sizeof(h_));
}

void FrameSectionWriter::end(uint64_t checksum) {
  h_.stored_bytes = stored_;
  w_.rewrite(0, &h_, sizeof(h_));
  w_.end(checksum);
}

FrameSectionReader::FrameSectionReader(Reader& r, uint32_t id, uint64_t expect_frames) : r_(r) {
  const SectionEntry& e = r.need(id);
  if (e.bytes < sizeof(FrameHeader)) fail("frame section " + std::to_string(id) + " is shorter than its header");
  r.seek(e.offset);
  r.read(&h_, sizeof(h_));
  if (h_.codec != QLX_FRAME_CODEC_RAW && h_.codec != QLX_FRAME_CODEC_BITMAP) fail("unknown frame codec " + std::to_string(h_.codec));
  if (h_.n_frames != expect_frames)
    fail("frame section " + std::to_string(id) + " holds " + std::to_string(h_.n_frames) + " frames, the state needs " +
         std::to_string(expect_frames));
  if (h_.chunk_frames == 0 || h_.chunk_frames > kMaxChunkFrames) fail("frame section chunk size outside 1.." + std::to_string(kMaxChunkFrames));
  if (h_.raw_bytes != h_.n_frames * kFrameBytes || h_.stored_bytes != e.bytes - sizeof(FrameHeader))
    fail("frame section " + std::to_string(id) + " sizes disagree");
  if (h_.codec == QLX_FRAME_CODEC_RAW && h_.stored_bytes != h_.raw_bytes) fail("raw frame section size disagrees with its frame count");
  checksum_ = e.checksum;
  left_ = h_.stored_bytes;
}

uint32_t FrameSectionReader::next_chunk(uint8_t* buf, uint64_t* bytes) {
  if (left_ < sizeof(ChunkHeader)) fail("frame section ends inside a chunk header");
  ChunkHeader c;
  r_.read(&c, sizeof(c));
  const uint64_t want = std::min<uint64_t>(h_.chunk_frames, frames_left());
  // every chunk but the last is full, so the frame count of each is known before it is read
  if (c.n_frames != want) fail("frame chunk n_frames " + std::to_string(c.n_frames) + ", expected " + std::to_string(want));
  if (c.value_bytes > (uint64_t)c.n_frames * kFrameBytes) fail("frame chunk value_bytes above its frames' size");
  const uint64_t total = chunk_fixed_bytes(c.n_frames) + c.value_bytes;
  if (total > left_) fail("frame chunk reaches past its section");
  std::memcpy(buf, &c, sizeof(c));
  r_.read(buf + sizeof(c), total - sizeof(c));
  validate_chunk(buf, total, h_.chunk_frames);
  left_ -= total;
  done_ += c.n_frames;
  *bytes = total;
  return c.n_frames;
}

void FrameSectionReader::next_raw(uint8_t* buf, uint32_t n) {
  const uint64_t bytes = (uint64_t)n * kFrameBytes;
  if (n > frames_left() || bytes > left_) fail("raw frame section is shorter than its frame count");
  r_.read(buf, bytes);
  left_ -= bytes;
  done_ += n;
}

void FrameSectionReader::finish() {
  if (done_ != h_.n_frames || left_ != 0) fail("frame section size disagrees with its frames");
}

void write_frames_host(Writer& w, uint32_t id, const uint8_t* frames, uint64_t n, uint32_t codec, uint32_t chunk_frames) {
  FrameSectionWriter fs(w, id, codec, chunk_frames, n);
  std::vector<uint8_t> buf(chunk_max_bytes(chunk_frames));
  for (uint64_t f = 0; f < n; f += chunk_frames) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk_frames, n - f);
    if (codec == QLX_FRAME_CODEC_BITMAP) fs.append(buf.data(), pack_chunk(frames + f * kFrameBytes, m, buf.data()));
    else fs.append(frames + f * kFrameBytes, (uint64_t)m * kFrameBytes);
  }
  fs.end(frame_checksum(frames, n, 0));
}

void read_frames_host(Reader& r, uint32_t id, uint64_t n, uint8_t* frames) {
  FrameSectionReader fs(r, id, n);
  const uint32_t C = fs.header().chunk_frames;
  std::vector<uint8_t> buf(chunk_max_bytes(C));
  uint64_t f = 0;
  while (fs.frames_left()) {
    uint32_t m;
    if (fs.header().codec == QLX_FRAME_CODEC_BITMAP) {
      uint64_t bytes;
      m = fs.next_chunk(buf.data(), &bytes);
      unpack_chunk(buf.data(), frames + f * kFrameBytes);
    } else {
      m = (uint32_t)std::min<uint64_t>(C, fs.frames_left());
      fs.next_raw(frames + f * kFrameBytes, m);
    }
    f += m;
  }
  fs.finish();
  if (frame_checksum(frames, n, 0) != fs.checksum()) fail("frame checksum mismatch in section " + std::to_string(id));
}

void read_info(const std::string& path, qlx_snapshot_info* out) {
  Reader r(path, 0);
  const std::vector<uint8_t> buf = r.small(SEC_INFO, sizeof(qlx_snapshot_info));
  if (buf.size() != sizeof(qlx_snapshot_info)) fail("info section of " + path + " has the wrong size");
  std::memcpy(out, buf.data(), sizeof(*out));
  if (out->format_version != r.header().version || out->kind != r.header().kind || out->file_bytes != r.header().file_bytes)
    fail("info section of " + path + " disagrees with the header");
}

}  // namespace snap
}  // namespace qlx
