// Frame sections of a snapshot on the device (frame_codec.hip): packing / unpacking kernels of QLX_FRAME_CODEC_BITMAP, the
// two-buffer pipeline between the GPU and the file, and the replay's sections, which the learner's snapshot reuses.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "objects.h"
#include "snapshot_format.h"

namespace qlx {

// `count` frames of a ring of `slots` frame slots, starting at slot `first` (wrapping): frame f lives at
// base + ((first + f) % slots) * 7056
struct FrameRing {
  uint8_t* base;
  uint64_t slots, first, count;
};

struct FrameIo {   // accumulated over the frame sections of one save or load
  uint64_t frames = 0, raw_bytes = 0, stored_bytes = 0;
  int codec = QLX_FRAME_CODEC_BITMAP;
  bool timing = false;        // QLX_SNAPSHOT_TIMING: HIP events around every chunk's codec kernels
  double kernel_us = 0.0;     // pack (save) or unpack (load) kernels' own time
  double hbm_bytes = 0.0;     // bytes those kernels read and wrote
};

// QLX_FRAME_CODEC_BITMAP unless QLX_SNAPSHOT_PACK=0 (read at every save)
int snapshot_codec_from_env();
// QLX_SNAPSHOT_TIMING=<file>: FrameIo::timing, and one JSON line per save / load appended to the file
void snapshot_timing_begin(FrameIo* io);
void snapshot_timing_report(const char* what, const FrameIo& io, double wall_s, uint64_t file_bytes);

void frames_write(snap::Writer& w, uint32_t id, const FrameRing& ring, hipStream_t s, FrameIo* io);
void frames_read(snap::Reader& r, uint32_t id, const FrameRing& ring, hipStream_t s, FrameIo* io);

// SEC_REPLAY + SEC_REPLAY_FRAMES of rb (the caller has synchronised whatever wrote it)
void replay_write(snap::Writer& w, qlx_replay* rb, hipStream_t s, FrameIo* io);
// capacity and n_envs of the replay a file holds
void replay_peek(snap::Reader& r, uint64_t* cap, uint32_t* n);
// fills a fresh replay of that capacity and n_envs; synchronises s
void replay_restore(snap::Reader& r, qlx_replay* rb, hipStream_t s, FrameIo* io);

// `count` elements of a device ring of `cap` elements from element `start` on (wrapping) <-> a host array
template <class T>
void ring_to_host(T* host, const T* dev, uint64_t cap, uint64_t start, uint64_t count) {
  const uint64_t a = std::min(count, cap - start);
  if (a) QLX_HIP(hipMemcpy(host, dev + start, a * sizeof(T), hipMemcpyDeviceToHost));
  if (count > a) QLX_HIP(hipMemcpy(host + a, dev, (count - a) * sizeof(T), hipMemcpyDeviceToHost));
}
template <class T>
void ring_from_host(T* dev, const T* host, uint64_t cap, uint64_t start, uint64_t count) {
  const uint64_t a = std::min(count, cap - start);
  if (a) QLX_HIP(hipMemcpy(dev + start, host, a * sizeof(T), hipMemcpyHostToDevice));
  if (count > a) QLX_HIP(hipMemcpy(dev, host + a, (count - a) * sizeof(T), hipMemcpyHostToDevice));
}

// runs f(), turning the container's FormatError into Error{QLX_E_IO}
template <class F>
void io_guard(F&& f) {
  try {
    f();
  } catch (const snap::FormatError& e) {
    throw Error{QLX_E_IO, e.msg};
  }
}

}  // namespace qlx
