// Host check of the snapshot container and of the bitmap codec's host reference (q-learning_amd/csrc/snapshot_format.cpp):
// a small container with both frame codecs is written and read back equal, and every corruption below must end in a
// FormatError (the library's QLX_E_IO), never in a sanitizer report.  Built host-only with AddressSanitizer and UBSan
// and run as a program (tests/test_snapshot_format.py):
//   hipcc --offload-host-only -x hip -I q-learning_amd/csrc -I include -fsanitize=address,undefined -g -O1 \
//         scripts/snapshot_host_check.cpp q-learning_amd/csrc/snapshot_format.cpp -o snapshot_host_check
//   ./snapshot_host_check <scratch dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "crc32c.h"
#include "snapshot_format.h"

using namespace qlx::snap;

static int g_fail = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

constexpr uint32_t kC = 3;        // chunk size of the test files
constexpr uint64_t kFrames = 8;   // chunks of 3, 3, 2
constexpr uint32_t kSecSmall = 40, kSecBitmap = 41, kSecRaw = 42;

static std::vector<uint8_t> make_frames() {
  std::vector<uint8_t> f(kFrames * kFrameBytes, 0);
  uint32_t x = 12345;
  auto rnd = [&] { x = x * 1664525u + 1013904223u; return x >> 8; };
  for (uint32_t i = 0; i < kFrameBytes; ++i) f[1 * kFrameBytes + i] = 255;                          // all non-zero
  f[2 * kFrameBytes] = 7;                                                                         // byte 0 only
  f[3 * kFrameBytes + kFrameBytes - 1] = 9;                                                       // byte 7,055 only
  for (uint32_t i = 0; i < 16; ++i) f[4 * kFrameBytes + 16 * 17 + i] = (uint8_t)(i + 1);          // one full group
  for (uint32_t i = 0; i < kFrameBytes; ++i) f[5 * kFrameBytes + i] = rnd() % 10 == 0 ? (uint8_t)(1 + rnd() % 255) : 0;
  for (uint32_t i = 0; i < kFrameBytes; ++i) f[6 * kFrameBytes + i] = (uint8_t)(1 + rnd() % 255);
  for (uint32_t i = 0; i < kFrameBytes; i += 97) f[7 * kFrameBytes + i] = 236;
  return f;                                                                                       // frame 0: all zero
}

static std::vector<uint8_t> read_file(const std::string& p) {
  std::vector<uint8_t> b;
  FILE* f = std::fopen(p.c_str(), "rb");
  if (!f) return b;
  std::fseek(f, 0, SEEK_END);
  b.resize((size_t)std::ftell(f));
  std::rewind(f);
  if (!b.empty() && std::fread(b.data(), 1, b.size(), f) != b.size()) b.clear();
  std::fclose(f);
  return b;
}

static void write_file(const std::string& p, const std::vector<uint8_t>& b) {
  FILE* f = std::fopen(p.c_str(), "wb");
  if (!f || std::fwrite(b.data(), 1, b.size(), f) != b.size()) { std::printf("cannot write %s\n", p.c_str()); std::exit(2); }
  std::fclose(f);
}

// reads everything the test file holds; returns the error text, empty when the file reads clean
static std::string read_all(const std::string& path, const std::vector<uint8_t>& small, const std::vector<uint8_t>& frames) {
  try {
    Reader r(path, QLX_SNAPSHOT_REPLAY);
    const std::vector<uint8_t> s = r.small(kSecSmall);
    std::vector<uint8_t> a(frames.size()), b(frames.size());
    read_frames_host(r, kSecBitmap, kFrames, a.data());
    read_frames_host(r, kSecRaw, kFrames, b.data());
    qlx_snapshot_info info;
    read_info(path, &info);
    if (s != small || a != frames || b != frames) return "read back differs";
    return "";
  } catch (const FormatError& e) {
    return e.msg.empty() ? "empty error" : e.msg;
  }
}

// the header's crc over a modified header / table, so that a test reaches the check behind it
static void fix_header_crc(std::vector<uint8_t>& file) {
  std::vector<uint8_t> h(file.begin(), file.begin() + kDataStart);
  std::memset(h.data() + 20, 0, 4);
  const uint32_t c = qlx::crc32c(h.data(), h.size());
  std::memcpy(file.data() + 20, &c, 4);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/check.qlx", bad = dir + "/bad.qlx";
  const std::vector<uint8_t> frames = make_frames();
  std::vector<uint8_t> small(1000);
  for (size_t i = 0; i < small.size(); ++i) small[i] = (uint8_t)(i * 31 + 7);

  // the codec alone
  {
    std::vector<uint8_t> buf(chunk_max_bytes(kFrames)), back(frames.size(), 0xA5);
    const uint64_t bytes = pack_chunk(frames.data(), kFrames, buf.data());
    uint64_t nnz = 0;
    for (uint8_t v : frames) nnz += v != 0;
    EXPECT(bytes == chunk_fixed_bytes(kFrames) + nnz);
    EXPECT(chunk_fixed_bytes(kFrames) == 8 + 16 + kFrames * 882);
    EXPECT(chunk_max_bytes(1) == 8 + 8 + 7938);
    validate_chunk(buf.data(), bytes, kFrames);
    unpack_chunk(buf.data(), back.data());
    EXPECT(back == frames);
    EXPECT(frame_checksum(frames.data(), kFrames, 0) ==
           frame_checksum(frames.data(), 3, 0) + frame_checksum(frames.data() + 3 * kFrameBytes, kFrames - 3, 3));
  }

  // write, read back equal; two writes are byte-identical; no .tmp is left
  auto write = [&](const std::string& p) {
    Writer w(p, QLX_SNAPSHOT_REPLAY);
    w.small(kSecSmall, small.data(), small.size());
    write_frames_host(w, kSecBitmap, frames.data(), kFrames, QLX_FRAME_CODEC_BITMAP, kC);
    write_frames_host(w, kSecRaw, frames.data(), kFrames, QLX_FRAME_CODEC_RAW, kC);
    qlx_snapshot_info info{};
    info.format_version = QLX_SNAPSHOT_VERSION;
    info.kind = QLX_SNAPSHOT_REPLAY;
    info.frames = 2 * kFrames;
    info.file_bytes = w.position() + sizeof(info);
    w.small(SEC_INFO, &info, sizeof(info));
    return w.finish();
  };
  const uint64_t size = write(path);
  const std::vector<uint8_t> good = read_file(path);
  EXPECT(good.size() == size && size > kDataStart);
  EXPECT(read_all(path, small, frames).empty());
  write(bad);
  EXPECT(read_file(bad) == good);
  EXPECT(read_file(path + ".tmp").empty() && read_file(bad + ".tmp").empty());
  {   // an abandoned writer leaves neither a file nor a .tmp
    { Writer w(dir + "/abandoned.qlx", QLX_SNAPSHOT_REPLAY); w.small(kSecSmall, small.data(), small.size()); }
    EXPECT(read_file(dir + "/abandoned.qlx").empty() && read_file(dir + "/abandoned.qlx.tmp").empty());
  }
  {   // wrong kind
    std::string msg;
    try { Reader r(path, QLX_SNAPSHOT_LEARNER); } catch (const FormatError& e) { msg = e.msg; }
    EXPECT(msg.find("kind") != std::string::npos);
  }

  // where the sections lie
  SectionEntry table[kMaxSections];
  std::memcpy(table, good.data() + sizeof(FileHeader), sizeof(table));
  uint32_t n_sections;
  std::memcpy(&n_sections, good.data() + 16, 4);
  EXPECT(n_sections == 4);
  const SectionEntry *e_small = nullptr, *e_bitmap = nullptr;
  for (uint32_t i = 0; i < n_sections; ++i) {
    if (table[i].id == kSecSmall) e_small = &table[i];
    if (table[i].id == kSecBitmap) e_bitmap = &table[i];
  }
  EXPECT(e_small && e_bitmap);
  if (!e_small || !e_bitmap) return 1;

  auto expect_error = [&](const char* what, const std::function<void(std::vector<uint8_t>&)>& corrupt, const char* needle) {
    std::vector<uint8_t> f = good;
    corrupt(f);
    write_file(bad, f);
    const std::string msg = read_all(bad, small, frames);
    const bool ok = !msg.empty() && msg != "read back differs" && (!needle || msg.find(needle) != std::string::npos);
    if (!ok) { std::printf("FAIL %s: got '%s'\n", what, msg.c_str()); ++g_fail; }
  };

  // truncation: at every section boundary, in the middle of every section, inside the header and the table, and empty
  std::vector<uint64_t> cuts = {0, 1, 8, 63, 64, 100, kDataStart - 1, kDataStart, size - 1};
  for (uint32_t i = 0; i < n_sections; ++i) {
    cuts.push_back(table[i].offset);
    cuts.push_back(table[i].offset + table[i].bytes / 2);
    cuts.push_back(table[i].offset + table[i].bytes - 1);
  }
  for (uint64_t c : cuts)
    if (c < size) expect_error(("truncation at " + std::to_string(c)).c_str(), [&](std::vector<uint8_t>& f) { f.resize(c); }, nullptr);
  // a truncated file whose header claims the shorter size: the section past the end is what is found
  expect_error("truncated with a matching header", [&](std::vector<uint8_t>& f) {
    const uint64_t c = size - 100;
    f.resize(c);
    std::memcpy(f.data() + 24, &c, 8);
    fix_header_crc(f);
  }, "past the end");
  expect_error("bad magic", [&](std::vector<uint8_t>& f) { f[3] ^= 1; }, "magic");
  expect_error("wrong version", [&](std::vector<uint8_t>& f) { const uint32_t v = QLX_SNAPSHOT_VERSION + 1; std::memcpy(f.data() + 8, &v, 4); fix_header_crc(f); }, "version");
  expect_error("header bit", [&](std::vector<uint8_t>& f) { f[sizeof(FileHeader) + 9] ^= 4; }, "header checksum");
  expect_error("section offset past the end", [&](std::vector<uint8_t>& f) {
    const uint64_t off = size + 1000;
    std::memcpy(f.data() + sizeof(FileHeader) + 8, &off, 8);
    fix_header_crc(f);
  }, "past the end");
  expect_error("section size past the end", [&](std::vector<uint8_t>& f) {
    const uint64_t bytes = ~0ull - 5;
    std::memcpy(f.data() + sizeof(FileHeader) + 16, &bytes, 8);
    fix_header_crc(f);
  }, "past the end");
  expect_error("flipped bit in a small section", [&](std::vector<uint8_t>& f) { f[e_small->offset + 500] ^= 0x10; }, "checksum mismatch in section");

  // the bitmap section's first chunk: header at +32, nnz at +40, masks after the padded table, then the values
  const uint64_t c0 = e_bitmap->offset + sizeof(FrameHeader);
  const uint64_t masks = c0 + chunk_mask_offset(kC), values = c0 + chunk_fixed_bytes(kC);
  expect_error("nnz disagrees with its mask", [&](std::vector<uint8_t>& f) { f[c0 + 8 + 2 * 2] ^= 1; }, "disagrees with its mask");
  expect_error("mask bit flipped", [&](std::vector<uint8_t>& f) { f[masks + 882 * 2 + 100] ^= 0x20; }, "disagrees with its mask");
  expect_error("nnz sum disagrees with value_bytes", [&](std::vector<uint8_t>& f) {
    // frame 0 of the chunk is all zero: give it one mask bit and nnz 1, so only the sum is off
    f[c0 + 8] = 1;
    f[masks] = 1;
  }, "nnz sum");
  expect_error("value_bytes changed", [&](std::vector<uint8_t>& f) { f[c0 + 4] ^= 1; }, nullptr);
  expect_error("n_frames above C", [&](std::vector<uint8_t>& f) { const uint32_t n = kC + 1; std::memcpy(f.data() + c0, &n, 4); }, "n_frames");
  expect_error("n_frames huge", [&](std::vector<uint8_t>& f) { const uint32_t n = 0xFFFFFFFFu; std::memcpy(f.data() + c0, &n, 4); }, "n_frames");
  expect_error("value_bytes huge", [&](std::vector<uint8_t>& f) { const uint32_t n = 0xFFFFFFF0u; std::memcpy(f.data() + c0 + 4, &n, 4); }, nullptr);
  expect_error("value flipped", [&](std::vector<uint8_t>& f) { f[values + 10] ^= 0x40; }, "frame checksum");
  expect_error("section chunk size zero", [&](std::vector<uint8_t>& f) { std::memset(f.data() + e_bitmap->offset + 4, 0, 4); }, "chunk size");
  expect_error("unknown codec", [&](std::vector<uint8_t>& f) { f[e_bitmap->offset] = 9; }, "codec");
  expect_error("frame count changed", [&](std::vector<uint8_t>& f) { f[e_bitmap->offset + 8] += 1; }, nullptr);

  // validate_chunk directly: n_frames above the caller's bound, and a chunk cut short
  {
    std::vector<uint8_t> buf(chunk_max_bytes(kC));
    const uint64_t bytes = pack_chunk(frames.data(), kC, buf.data());
    int caught = 0;
    try { validate_chunk(buf.data(), bytes, kC - 1); } catch (const FormatError&) { ++caught; }
    try { validate_chunk(buf.data(), bytes - 1, kC); } catch (const FormatError&) { ++caught; }
    try { validate_chunk(buf.data(), 4, kC); } catch (const FormatError&) { ++caught; }
    EXPECT(caught == 3);
  }

  std::remove(path.c_str());
  std::remove(bad.c_str());
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
