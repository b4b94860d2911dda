// Snapshot frame sections on the GPU (gfx950): the QLX_FRAME_CODEC_BITMAP kernels, the frame checksum, the two-buffer
// pipeline between HBM and the file, the replay's sections and the replay / codec entry points.
//
// A frame is 7,056 bytes = 441 groups of 16 bytes; Breakout frames are about 10 % non-zero with four distinct values
// (DESIGN.md "Snapshots"), so a frame packs into its 882-byte bitmap plus its non-zero bytes.  Per chunk of up to C frames
// (layout: snapshot_format.h) four launches, no data passing between workgroups inside a launch:
//   k_frame_checksum  per-frame partial of the section checksum over the raw frames
//   k_codec_count     one pass: 16-byte loads, the 16-bit non-zero mask of each group -> the bitmap, popcounts -> nnz
//   k_codec_scan      one workgroup: exclusive scan of the chunk's nnz -> each frame's value offset (+ the chunk header)
//   k_codec_pack      per frame, an in-frame scan of the groups' popcounts (wave shuffles + LDS wave totals) gives every
//                     group its value offset; values are stored byte by byte, so any offset is correct
// and k_codec_unpack, the reverse of the last (zero-filling).  441 is no multiple of 64 or 256: every thread takes part in
// both rounds of the in-frame scan and only the loads and stores are masked.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "frame_codec.h"

namespace qlx {

namespace {

constexpr int kGroups = kFramePix / 16;   // 441
constexpr int kCodecThreads = 256;
constexpr int kRounds = (kGroups + kCodecThreads - 1) / kCodecThreads;   // 2
static_assert(kFramePix == (int)snap::kFrameBytes && kGroups * 2 == (int)snap::kMaskBytes, "frame geometry");

__device__ __forceinline__ const uint8_t* ring_frame(const uint8_t* base, uint64_t slots, uint64_t first, uint32_t f) {
  return base + ((first + f) % slots) * (uint64_t)kFramePix;
}

// bit i = byte i of the 16-byte group is non-zero
__device__ __forceinline__ uint32_t nz_mask16(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t x = w[i];
    const uint32_t b = ((x & 0xFFu) ? 1u : 0u) | ((x & 0xFF00u) ? 2u : 0u) | ((x & 0xFF0000u) ? 4u : 0u) | ((x & 0xFF000000u) ? 8u : 0u);
    m |= b << (4 * i);
  }
  return m;
}

// exclusive prefix of v over the 256 threads of the block and the block's total; every thread calls it
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wave_tot, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kCodecThreads / 64; ++w) {
    before += w < wave ? wave_tot[w] : 0u;
    tot += wave_tot[w];
  }
  __syncthreads();   // wave_tot is read before the next call writes it
  *total = tot;
  return before + inc - v;
}

// partial[f] = sum over the frame's 8-byte words w_k of w_k * ((2 j + 1) * kH1), j = (ordinal + f) * 882 + k
__global__ __launch_bounds__(kCodecThreads) void k_frame_checksum(const uint8_t* base, uint64_t slots, uint64_t first, uint32_t n,
                                                                   uint64_t ordinal, unsigned long long* partial) {
  __shared__ unsigned long long red[kCodecThreads];
  const uint32_t f = blockIdx.x;
  const uint4* src = reinterpret_cast<const uint4*>(ring_frame(base, slots, first, f));
  unsigned long long sum = 0;
  for (int g = threadIdx.x; g < kGroups; g += kCodecThreads) {
    const uint4 v = src[g];
    const unsigned long long lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    const unsigned long long hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    const unsigned long long j = (ordinal + f) * (unsigned long long)snap::kFrameWords + 2ull * g;
    sum += lo * ((2 * j + 1) * snap::kChecksumMul) + hi * ((2 * j + 3) * snap::kChecksumMul);
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int d = kCodecThreads / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[f] = red[0];
}

// masks [n][882] and nnz [n] (u16) of the chunk's frames
__global__ __launch_bounds__(kCodecThreads) void k_codec_count(const uint8_t* base, uint64_t slots, uint64_t first, uint32_t n,
                                                                uint8_t* chunk, uint32_t mask_off) {
  __shared__ uint32_t wave_tot[kCodecThreads / 64];
  const uint32_t f = blockIdx.x;
  const uint4* src = reinterpret_cast<const uint4*>(ring_frame(base, slots, first, f));
  uint16_t* mask = reinterpret_cast<uint16_t*>(chunk + mask_off + (size_t)f * snap::kMaskBytes);
  uint32_t cnt = 0;
  for (int g = threadIdx.x; g < kGroups; g += kCodecThreads) {
    const uint32_t m = nz_mask16(src[g]);
    mask[g] = (uint16_t)m;
    cnt += (uint32_t)__popc(m);
  }
  uint32_t total;
  block_exclusive_scan(cnt, wave_tot, &total);
  if (threadIdx.x == 0) reinterpret_cast<uint16_t*>(chunk + sizeof(snap::ChunkHeader))[f] = (uint16_t)total;
}

// one wave: off[f] = sum of nnz[0..f); write_header: the chunk header and the zero padding of the nnz table
__global__ __launch_bounds__(64) void k_codec_scan(uint8_t* chunk, uint32_t n, uint32_t mask_off, uint32_t* off, int write_header) {
  const uint16_t* nnz = reinterpret_cast<const uint16_t*>(chunk + sizeof(snap::ChunkHeader));
  const int lane = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t b = 0; b < n; b += 64) {
    const uint32_t i = b + lane;
    const uint32_t v = i < n ? nnz[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (i < n) off[i] = carry + inc - v;
    carry += __shfl(inc, 63);
  }
  if (write_header && lane == 0) {
    uint32_t* h = reinterpret_cast<uint32_t*>(chunk);
    h[0] = n;
    h[1] = carry;
    for (uint32_t i = (uint32_t)sizeof(snap::ChunkHeader) + 2 * n; i < mask_off; ++i) chunk[i] = 0;
  }
}

__global__ __launch_bounds__(kCodecThreads) void k_codec_pack(const uint8_t* base, uint64_t slots, uint64_t first, uint32_t n,
                                                               const uint32_t* off, uint8_t* values) {
  __shared__ uint32_t wave_tot[kCodecThreads / 64];
  const uint32_t f = blockIdx.x;
  const uint4* src = reinterpret_cast<const uint4*>(ring_frame(base, slots, first, f));
  uint32_t at = off[f];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int g = r * kCodecThreads + (int)threadIdx.x;
    const uint4 v = g < kGroups ? src[g] : make_uint4(0, 0, 0, 0);
    const uint32_t m = nz_mask16(v);
    uint32_t total;
    uint32_t o = at + block_exclusive_scan((uint32_t)__popc(m), wave_tot, &total);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((m >> i) & 1u) values[o++] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    at += total;
  }
}

__global__ __launch_bounds__(kCodecThreads) void k_codec_unpack(const uint8_t* chunk, uint32_t mask_off, const uint32_t* off,
                                                                 const uint8_t* values, uint8_t* base, uint64_t slots, uint64_t first,
                                                                 uint32_t n) {
  __shared__ uint32_t wave_tot[kCodecThreads / 64];
  const uint32_t f = blockIdx.x;
  uint4* dst = reinterpret_cast<uint4*>(const_cast<uint8_t*>(ring_frame(base, slots, first, f)));
  const uint16_t* mask = reinterpret_cast<const uint16_t*>(chunk + mask_off + (size_t)f * snap::kMaskBytes);
  uint32_t at = off[f];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int g = r * kCodecThreads + (int)threadIdx.x;
    const uint32_t m = g < kGroups ? mask[g] : 0u;
    uint32_t total;
    uint32_t o = at + block_exclusive_scan((uint32_t)__popc(m), wave_tot, &total);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((m >> i) & 1u) w[i >> 2] |= (uint32_t)values[o++] << (8 * (i & 3));
    if (g < kGroups) dst[g] = make_uint4(w[0], w[1], w[2], w[3]);
    at += total;
  }
}

// ---- the pipeline ----
using Sink = std::function<void(const uint8_t* data, uint64_t bytes)>;
// the next `want` frames into buf: a validated chunk (bitmap; *bytes = its size) or the raw frames
using Source = std::function<void(uint8_t* buf, uint64_t* bytes, uint32_t want)>;

// two of every buffer a chunk in flight needs; the destructor waits for the stream before anything is freed
struct Pipe {
  hipStream_t s;
  bool timing;
  DeviceBuffer<uint8_t> d_chunk[2];
  DeviceBuffer<uint32_t> d_off[2];
  DeviceBuffer<unsigned long long> d_part[2];
  PinnedBuffer<uint8_t> h_chunk[2];
  PinnedBuffer<unsigned long long> h_part[2];
  PinnedBuffer<snap::ChunkHeader> h_hdr;
  hipEvent_t ev_packed[2] = {}, ev_done[2] = {}, t0[2] = {}, t1[2] = {};
  Pipe(uint32_t C, bool bitmap, hipStream_t s_, bool timing_) : s(s_), timing(timing_) {
    try {
      const size_t bytes = bitmap ? snap::chunk_max_bytes(C) : (size_t)C * kFramePix;
      for (int b = 0; b < 2; ++b) {
        if (bitmap) {
          d_chunk[b].alloc(bytes);
          d_off[b].alloc(C);
        }
        d_part[b].alloc(C);
        h_chunk[b].alloc(bytes);
        h_part[b].alloc(C);
        QLX_HIP(hipEventCreateWithFlags(&ev_packed[b], hipEventDisableTiming));
        QLX_HIP(hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming));
        if (timing) {
          QLX_HIP(hipEventCreate(&t0[b]));
          QLX_HIP(hipEventCreate(&t1[b]));
        }
      }
      h_hdr.alloc(2);
    } catch (...) {
      destroy_events();
      throw;
    }
  }
  ~Pipe() {
    (void)hipStreamSynchronize(s);
    destroy_events();
  }
  void destroy_events() {
    for (int b = 0; b < 2; ++b)
      for (hipEvent_t* e : {&ev_packed[b], &ev_done[b], &t0[b], &t1[b]})
        if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
  }
  double elapsed_us(int b) {
    float ms = 0.0f;
    QLX_HIP(hipEventElapsedTime(&ms, t0[b], t1[b]));
    return ms * 1000.0;
  }
};

// frames [f0, f0 + m) of the ring <-> a host buffer, in at most two pieces
void ring_copy_async(const FrameRing& ring, uint64_t f0, uint32_t m, uint8_t* host, bool to_host, hipStream_t s) {
  const uint64_t first = (ring.first + f0) % ring.slots;
  const uint64_t a = std::min<uint64_t>(m, ring.slots - first);
  uint8_t* d0 = ring.base + first * kFramePix;
  if (to_host) {
    QLX_HIP(hipMemcpyAsync(host, d0, a * kFramePix, hipMemcpyDeviceToHost, s));
    if (m > a) QLX_HIP(hipMemcpyAsync(host + a * kFramePix, ring.base, (m - a) * kFramePix, hipMemcpyDeviceToHost, s));
  } else {
    QLX_HIP(hipMemcpyAsync(d0, host, a * kFramePix, hipMemcpyHostToDevice, s));
    if (m > a) QLX_HIP(hipMemcpyAsync(ring.base, host + a * kFramePix, (m - a) * kFramePix, hipMemcpyHostToDevice, s));
  }
}

void launch_checksum(const FrameRing& ring, uint64_t f0, uint32_t m, unsigned long long* d_part, hipStream_t s) {
  hipLaunchKernelGGL(k_frame_checksum, dim3(m), dim3(kCodecThreads), 0, s, ring.base, ring.slots, (ring.first + f0) % ring.slots, m, f0,
                     d_part);
  QLX_HIP(hipGetLastError());
}

// ring -> sink, chunk by chunk: chunk k is packed on the stream and copied into pinned buffer k & 1 while the host hands
// buffer (k - 1) & 1 to the sink.  Returns the checksum of the raw frames (computed before packing).
uint64_t pack_stream(const FrameRing& ring, int codec, uint32_t C, hipStream_t s, const Sink& sink, FrameIo* io) {
  if (ring.count == 0) return 0;
  const bool bitmap = codec == QLX_FRAME_CODEC_BITMAP;
  Pipe p(C, bitmap, s, io && io->timing && bitmap);
  const uint64_t chunks = (ring.count + C - 1) / C;
  auto frames_of = [&](uint64_t k) { return (uint32_t)std::min<uint64_t>(C, ring.count - k * C); };
  auto enqueue = [&](uint64_t k) {
    const int b = (int)(k & 1);
    const uint32_t m = frames_of(k);
    const uint64_t f0 = k * C, first = (ring.first + f0) % ring.slots;
    launch_checksum(ring, f0, m, p.d_part[b], s);
    if (bitmap) {
      const uint32_t mask_off = (uint32_t)snap::chunk_mask_offset(m);
      if (p.timing) QLX_HIP(hipEventRecord(p.t0[b], s));
      hipLaunchKernelGGL(k_codec_count, dim3(m), dim3(kCodecThreads), 0, s, ring.base, ring.slots, first, m, p.d_chunk[b].get(), mask_off);
      hipLaunchKernelGGL(k_codec_scan, dim3(1), dim3(64), 0, s, p.d_chunk[b].get(), m, mask_off, p.d_off[b].get(), 1);
      hipLaunchKernelGGL(k_codec_pack, dim3(m), dim3(kCodecThreads), 0, s, ring.base, ring.slots, first, m, p.d_off[b].get(),
                         p.d_chunk[b] + snap::chunk_fixed_bytes(m));
      QLX_HIP(hipGetLastError());
      if (p.timing) QLX_HIP(hipEventRecord(p.t1[b], s));
      QLX_HIP(hipMemcpyAsync(p.h_hdr + b, p.d_chunk[b], sizeof(snap::ChunkHeader), hipMemcpyDeviceToHost, s));
    }
    QLX_HIP(hipMemcpyAsync(p.h_part[b], p.d_part[b], m * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    QLX_HIP(hipEventRecord(p.ev_packed[b], s));
  };
  uint64_t sum = 0, prev_bytes = 0;
  enqueue(0);
  for (uint64_t k = 0; k < chunks; ++k) {
    const int b = (int)(k & 1);
    const uint32_t m = frames_of(k);
    QLX_HIP(hipEventSynchronize(p.ev_packed[b]));
    for (uint32_t f = 0; f < m; ++f) sum += p.h_part[b][f];
    uint64_t bytes = (uint64_t)m * kFramePix;
    if (bitmap) {
      const snap::ChunkHeader h = p.h_hdr[b];
      QLX_CHECK(h.n_frames == m && h.value_bytes <= (uint64_t)m * kFramePix, QLX_E_STATE, "frame codec: the packed chunk header is inconsistent");
      bytes = snap::chunk_fixed_bytes(m) + h.value_bytes;
      QLX_HIP(hipMemcpyAsync(p.h_chunk[b], p.d_chunk[b], bytes, hipMemcpyDeviceToHost, s));
      if (p.timing) {
        io->kernel_us += p.elapsed_us(b);
        io->hbm_bytes += 2.0 * m * kFramePix + (double)bytes;   // the frames read twice, the chunk written
      }
    } else {
      ring_copy_async(ring, k * C, m, p.h_chunk[b], true, s);
    }
    QLX_HIP(hipEventRecord(p.ev_done[b], s));
    if (k + 1 < chunks) enqueue(k + 1);
    if (k > 0) {
      QLX_HIP(hipEventSynchronize(p.ev_done[b ^ 1]));
      sink(p.h_chunk[b ^ 1], prev_bytes);
    }
    prev_bytes = bytes;
  }
  const int last = (int)((chunks - 1) & 1);
  QLX_HIP(hipEventSynchronize(p.ev_done[last]));
  sink(p.h_chunk[last], prev_bytes);
  return sum;
}

// source -> ring, the same pipeline in reverse: the host reads (and validates) chunk k into pinned buffer k & 1 while the
// GPU unpacks chunk k - 1.  Returns the checksum of the frames as they stand in the ring after unpacking.
uint64_t unpack_stream(const FrameRing& ring, int codec, uint32_t C, hipStream_t s, const Source& source, FrameIo* io) {
  if (ring.count == 0) return 0;
  const bool bitmap = codec == QLX_FRAME_CODEC_BITMAP;
  Pipe p(C, bitmap, s, io && io->timing && bitmap);
  const uint64_t chunks = (ring.count + C - 1) / C;
  auto frames_of = [&](uint64_t k) { return (uint32_t)std::min<uint64_t>(C, ring.count - k * C); };
  uint64_t sum = 0;
  auto retire = [&](uint64_t k) {   // chunk k is on the device and summed
    const int b = (int)(k & 1);
    QLX_HIP(hipEventSynchronize(p.ev_done[b]));
    for (uint32_t f = 0; f < frames_of(k); ++f) sum += p.h_part[b][f];
    if (p.timing) io->kernel_us += p.elapsed_us(b);
  };
  for (uint64_t k = 0; k < chunks; ++k) {
    const int b = (int)(k & 1);
    const uint32_t m = frames_of(k);
    const uint64_t f0 = k * C;
    if (k >= 2) retire(k - 2);
    uint64_t bytes = 0;
    source(p.h_chunk[b], &bytes, m);   // validated: nothing below depends on an unchecked byte of the file
    if (bitmap) {
      const uint32_t mask_off = (uint32_t)snap::chunk_mask_offset(m);
      QLX_HIP(hipMemcpyAsync(p.d_chunk[b], p.h_chunk[b], bytes, hipMemcpyHostToDevice, s));
      if (p.timing) QLX_HIP(hipEventRecord(p.t0[b], s));
      hipLaunchKernelGGL(k_codec_scan, dim3(1), dim3(64), 0, s, p.d_chunk[b].get(), m, mask_off, p.d_off[b].get(), 0);
      hipLaunchKernelGGL(k_codec_unpack, dim3(m), dim3(kCodecThreads), 0, s, p.d_chunk[b].get(), mask_off, p.d_off[b].get(),
                         p.d_chunk[b] + snap::chunk_fixed_bytes(m), ring.base, ring.slots, (ring.first + f0) % ring.slots, m);
      QLX_HIP(hipGetLastError());
      if (p.timing) {
        QLX_HIP(hipEventRecord(p.t1[b], s));
        io->hbm_bytes += (double)m * kFramePix + (double)bytes;   // the chunk read, the frames written
      }
    } else {
      ring_copy_async(ring, f0, m, p.h_chunk[b], false, s);
    }
    launch_checksum(ring, f0, m, p.d_part[b], s);
    QLX_HIP(hipMemcpyAsync(p.h_part[b], p.d_part[b], m * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    QLX_HIP(hipEventRecord(p.ev_done[b], s));
  }
  if (chunks >= 2) retire(chunks - 2);
  retire(chunks - 1);
  return sum;
}

struct ReplayMeta {
  uint64_t cap, n, total, len, frame_first, frame_count;
};
static_assert(sizeof(ReplayMeta) == 48, "replay section header");

uint64_t replay_meta_bytes(uint64_t len) { return sizeof(ReplayMeta) + ((2 * len + 3) & ~3ull) + 8 * len; }

struct StreamSync {   // a failed restore leaves no work in flight on the object it was filling
  hipStream_t s;
  ~StreamSync() { (void)hipStreamSynchronize(s); }
};

}  // namespace

int snapshot_codec_from_env() {
  const char* v = std::getenv("QLX_SNAPSHOT_PACK");
  return (v && v[0] == '0') ? QLX_FRAME_CODEC_RAW : QLX_FRAME_CODEC_BITMAP;
}

void snapshot_timing_begin(FrameIo* io) {
  const char* v = std::getenv("QLX_SNAPSHOT_TIMING");
  io->timing = v && v[0];
}

void snapshot_timing_report(const char* what, const FrameIo& io, double wall_s, uint64_t file_bytes) {
  if (!io.timing) return;
  FILE* f = std::fopen(std::getenv("QLX_SNAPSHOT_TIMING"), "a");
  if (!f) return;
  std::fprintf(f, "{\"op\": \"%s\", \"codec\": %d, \"wall_s\": %.6f, \"file_bytes\": %llu, \"frames\": %llu, \"frame_bytes_raw\": %llu, "
                  "\"frame_bytes_stored\": %llu, \"kernel_us\": %.3f, \"kernel_hbm_bytes\": %.0f}\n",
               what, io.codec, wall_s, (unsigned long long)file_bytes, (unsigned long long)io.frames, (unsigned long long)io.raw_bytes,
               (unsigned long long)io.stored_bytes, io.kernel_us, io.hbm_bytes);
  std::fclose(f);
}

void frames_write(snap::Writer& w, uint32_t id, const FrameRing& ring, hipStream_t s, FrameIo* io) {
  snap::FrameSectionWriter fs(w, id, (uint32_t)io->codec, snap::kChunkFrames, ring.count);
  const uint64_t sum = pack_stream(ring, io->codec, snap::kChunkFrames, s, [&](const uint8_t* d, uint64_t b) { fs.append(d, b); }, io);
  fs.end(sum);
  io->frames += ring.count;
  io->raw_bytes += ring.count * kFramePix;
  io->stored_bytes += fs.stored();
}

void frames_read(snap::Reader& r, uint32_t id, const FrameRing& ring, hipStream_t s, FrameIo* io) {
  snap::FrameSectionReader fs(r, id, ring.count);
  const snap::FrameHeader h = fs.header();
  io->codec = (int)h.codec;
  const uint64_t sum = unpack_stream(ring, (int)h.codec, h.chunk_frames, s, [&](uint8_t* buf, uint64_t* bytes, uint32_t want) {
    if (h.codec == QLX_FRAME_CODEC_BITMAP) {
      const uint32_t got = fs.next_chunk(buf, bytes);
      if (got != want) throw snap::FormatError{"snapshot: frame chunk holds another frame count than its place in the section"};
    } else {
      fs.next_raw(buf, want);
      *bytes = (uint64_t)want * kFramePix;
    }
  }, io);
  fs.finish();
  if (sum != fs.checksum()) throw snap::FormatError{"snapshot: frame checksum mismatch in section " + std::to_string(id)};
  io->frames += ring.count;
  io->raw_bytes += h.raw_bytes;
  io->stored_bytes += h.stored_bytes;
}

void replay_write(snap::Writer& w, qlx_replay* rb, hipStream_t s, FrameIo* io) {
  const uint64_t len = rb->len(), start = (rb->total - len) % rb->cap;
  ReplayMeta m{rb->cap, rb->n, rb->total, len, 0, std::min<uint64_t>(rb->total, rb->F)};
  m.frame_first = rb->total - m.frame_count;
  std::vector<uint8_t> buf(replay_meta_bytes(len), 0);
  std::memcpy(buf.data(), &m, sizeof(m));
  uint8_t* act = buf.data() + sizeof(m);
  uint8_t* done = act + len;
  float* rew = reinterpret_cast<float*>(buf.data() + sizeof(m) + ((2 * len + 3) & ~3ull));
  uint32_t* eps = reinterpret_cast<uint32_t*>(rew + len);
  if (len) {
    ring_to_host(act, rb->d_action.get(), rb->cap, start, len);
    ring_to_host(done, rb->d_done.get(), rb->cap, start, len);
    ring_to_host(rew, rb->d_reward.get(), rb->cap, start, len);
    ring_to_host(eps, rb->d_epstep.get(), rb->cap, start, len);
  }
  w.small(snap::SEC_REPLAY, buf.data(), buf.size());
  // the newest min(total, F) push positions: a transition's s reaches back at most 4 n positions (replay_dev.h), so these
  // are all the frames replay_frames can address
  frames_write(w, snap::SEC_REPLAY_FRAMES, FrameRing{rb->d_frames, rb->F, m.frame_first % rb->F, m.frame_count}, s, io);
}

static ReplayMeta replay_meta(const std::vector<uint8_t>& buf) {
  if (buf.size() < sizeof(ReplayMeta)) throw snap::FormatError{"snapshot: replay section shorter than its header"};
  ReplayMeta m;
  std::memcpy(&m, buf.data(), sizeof(m));
  const bool ok = m.cap > 0 && m.n > 0 && m.n <= 0xFFFFFFFFull && m.cap < (1ull << 40) && m.len == std::min(m.total, m.cap) &&
                  m.frame_count == std::min(m.total, m.cap + 4 * m.n) && m.frame_first == m.total - m.frame_count &&
                  buf.size() == replay_meta_bytes(m.len);
  if (!ok) throw snap::FormatError{"snapshot: replay section is inconsistent"};
  return m;
}

void replay_peek(snap::Reader& r, uint64_t* cap, uint32_t* n) {
  // the header alone (the section's crc is checked when it is restored)
  const snap::SectionEntry& e = r.need(snap::SEC_REPLAY);
  if (e.bytes < sizeof(ReplayMeta)) throw snap::FormatError{"snapshot: replay section shorter than its header"};
  ReplayMeta m;
  r.seek(e.offset);
  r.read(&m, sizeof(m));
  if (m.cap == 0 || m.n == 0 || m.n > 0xFFFFFFFFull || m.cap >= (1ull << 40) || e.bytes != replay_meta_bytes(std::min(m.total, m.cap)))
    throw snap::FormatError{"snapshot: replay section is inconsistent"};
  *cap = m.cap;
  *n = (uint32_t)m.n;
}

void replay_restore(snap::Reader& r, qlx_replay* rb, hipStream_t s, FrameIo* io) {
  StreamSync sync{s};
  const std::vector<uint8_t> buf = r.small(snap::SEC_REPLAY);
  const ReplayMeta m = replay_meta(buf);
  if (m.cap != rb->cap || m.n != rb->n) throw snap::FormatError{"snapshot: replay capacity / n_envs disagree with the learner's parameters"};
  const uint64_t len = m.len, start = (m.total - len) % m.cap;
  const uint8_t* act = buf.data() + sizeof(m);
  const uint8_t* done = act + len;
  const float* rew = reinterpret_cast<const float*>(buf.data() + sizeof(m) + ((2 * len + 3) & ~3ull));
  const uint32_t* eps = reinterpret_cast<const uint32_t*>(rew + len);
  if (len) {
    ring_from_host(rb->d_action.get(), act, m.cap, start, len);
    ring_from_host(rb->d_done.get(), done, m.cap, start, len);
    ring_from_host(rb->d_reward.get(), rew, m.cap, start, len);
    ring_from_host(rb->d_epstep.get(), eps, m.cap, start, len);
  }
  frames_read(r, snap::SEC_REPLAY_FRAMES, FrameRing{rb->d_frames, rb->F, m.frame_first % rb->F, m.frame_count}, s, io);
  rb->total = m.total;
}

}  // namespace qlx

using namespace qlx;

extern "C" {

int32_t qlx_snapshot_info_read(const char* path, qlx_snapshot_info* out) {
  return guard([&] {
    QLX_CHECK(path && out, QLX_E_INVALID, "null argument");
    io_guard([&] { snap::read_info(path, out); });
  });
}

int32_t qlx_replay_save(qlx_replay* rb, const char* path) {
  return guard([&] {
    QLX_CHECK(rb && path, QLX_E_INVALID, "null argument");
    QLX_HIP(hipSetDevice(rb->device));
    QLX_HIP(hipDeviceSynchronize());   // pushes run on the env's stream
    const auto t0 = std::chrono::steady_clock::now();
    FrameIo io;
    io.codec = snapshot_codec_from_env();
    snapshot_timing_begin(&io);
    uint64_t file_bytes = 0;
    io_guard([&] {
      snap::Writer w(path, QLX_SNAPSHOT_REPLAY);
      replay_write(w, rb, rb->stream, &io);
      qlx_snapshot_info info{};
      info.format_version = QLX_SNAPSHOT_VERSION;
      info.kind = QLX_SNAPSHOT_REPLAY;
      info.frame_codec = (uint32_t)io.codec;
      info.replay_len = rb->len();
      info.replay_total = rb->total;
      info.frames = io.frames;
      info.frame_bytes_raw = io.raw_bytes;
      info.frame_bytes_stored = io.stored_bytes;
      info.file_bytes = w.position() + sizeof(info);
      info.params.n_envs = rb->n;
      info.params.history_buffer_len = rb->cap;
      w.small(snap::SEC_INFO, &info, sizeof(info));
      file_bytes = w.finish();
    });
    snapshot_timing_report("replay_save", io, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), file_bytes);
  });
}

int32_t qlx_replay_load(const char* path, int32_t device, qlx_replay** out) {
  return guard([&] {
    QLX_CHECK(path && out, QLX_E_INVALID, "null argument");
    const auto t0 = std::chrono::steady_clock::now();
    FrameIo io;
    snapshot_timing_begin(&io);
    io_guard([&] {
      snap::Reader r(path, QLX_SNAPSHOT_REPLAY);
      uint64_t cap = 0;
      uint32_t n = 0;
      replay_peek(r, &cap, &n);
      qlx_replay* rb = nullptr;
      const int32_t st = qlx_replay_create(cap, n, device, &rb);
      QLX_CHECK(st == QLX_OK, st, qlx_last_error());
      try {
        replay_restore(r, rb, rb->stream, &io);
      } catch (...) {
        qlx_replay_destroy(rb);
        throw;
      }
      *out = rb;
      snapshot_timing_report("replay_load", io, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                             r.header().file_bytes);
    });
  });
}

int32_t qlx_frame_codec_roundtrip(const uint8_t* frames, uint32_t n, int32_t codec, int32_t device, uint8_t* packed_out, uint64_t cap,
                                  uint64_t* packed_bytes, uint8_t* frames_out) {
  return guard([&] {
    QLX_CHECK(frames && packed_out && packed_bytes && frames_out && n > 0, QLX_E_INVALID, "null argument or n = 0");
    QLX_CHECK(codec == QLX_FRAME_CODEC_RAW || codec == QLX_FRAME_CODEC_BITMAP, QLX_E_INVALID, "unknown frame codec");
    current_device_checked(device);
    struct Stream {
      hipStream_t s = nullptr;
      ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    } st;
    QLX_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    const size_t bytes = (size_t)n * kFramePix;
    DeviceBuffer<uint8_t> d_in(bytes), d_out(bytes);
    QLX_HIP(hipMemcpy(d_in, frames, bytes, hipMemcpyHostToDevice));
    QLX_HIP(hipMemset(d_out, 0xA5, bytes));   // unpacking must write the zeros too
    const uint32_t C = snap::kChunkFrames;
    uint64_t at = 0;
    const uint64_t sum_in = pack_stream(FrameRing{d_in, n, 0, n}, codec, C, st.s, [&](const uint8_t* d, uint64_t b) {
      QLX_CHECK(at + b <= cap, QLX_E_INVALID, "packed_out is too small");
      std::memcpy(packed_out + at, d, b);
      at += b;
    }, nullptr);
    *packed_bytes = at;
    uint64_t rd = 0;
    uint64_t sum_out = 0;
    io_guard([&] {
      sum_out = unpack_stream(FrameRing{d_out, n, 0, n}, codec, C, st.s, [&](uint8_t* buf, uint64_t* nbytes, uint32_t want) {
        uint64_t total = (uint64_t)want * kFramePix;
        if (codec == QLX_FRAME_CODEC_BITMAP) {
          snap::ChunkHeader h;
          if (at - rd < sizeof(h)) throw snap::FormatError{"frame codec: packed stream ends inside a chunk header"};
          std::memcpy(&h, packed_out + rd, sizeof(h));
          if (h.n_frames != want || h.value_bytes > total) throw snap::FormatError{"frame codec: packed chunk header is inconsistent"};
          total = snap::chunk_fixed_bytes(want) + h.value_bytes;
        }
        if (at - rd < total) throw snap::FormatError{"frame codec: packed stream is short"};
        if (codec == QLX_FRAME_CODEC_BITMAP) snap::validate_chunk(packed_out + rd, total, C);
        std::memcpy(buf, packed_out + rd, total);
        rd += total;
        *nbytes = total;
      }, nullptr);
    });
    QLX_CHECK(sum_in == sum_out && rd == at, QLX_E_IO, "frame codec: checksum of the unpacked frames differs from the input's");
    QLX_HIP(hipMemcpy(frames_out, d_out, bytes, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
