// Snapshots of the Breakout learner (DESIGN.md "Snapshots"): qlx_learner_save / qlx_learner_load.
// Everything the next vector step reads: params and host counters, the env (mechanics, episode steps, checksums, ring
// frames), the replay (replay_write), both models, the episode books, the prioritized-replay leaves and the target memo.
// Every draw is a function of those counters, so a loaded learner continues bit for bit.  Small sections are built on
// the host and carry a crc32c; frames go through the frame codec (frame_codec.hip).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "frame_codec.h"
#include "learner.h"
#include "qnet.h"

using namespace qlx;

namespace {

constexpr uint64_t kModelSectionBytes = 8 + 3 * (uint64_t)kNumParams * sizeof(float);

void model_section_write(snap::Writer& w, uint32_t id, qlx_model* m) {
  snap::Blob b;
  uint8_t* p = b.grow(kModelSectionBytes);
  int64_t it = 0;
  model_state_get(m, reinterpret_cast<float*>(p + 8), &it);
  std::memcpy(p, &it, 8);
  w.small(id, b.bytes.data(), b.bytes.size());
}

void model_section_read(snap::Reader& r, uint32_t id, qlx_model* m) {
  const std::vector<uint8_t> buf = r.small(id, kModelSectionBytes);
  if (buf.size() != kModelSectionBytes) throw snap::FormatError{"snapshot: model section " + std::to_string(id) + " has the wrong size"};
  int64_t it = 0;
  std::memcpy(&it, buf.data(), 8);
  model_state_put(m, reinterpret_cast<const float*>(buf.data() + 8), it);
}

template <class T>
void put_device(snap::Blob& b, const T* dev, uint64_t count) {
  if (count) QLX_HIP(hipMemcpy(b.grow(count * sizeof(T)), dev, count * sizeof(T), hipMemcpyDeviceToHost));
}
template <class T>
void get_device(snap::BlobReader& br, T* dev, uint64_t count) {
  if (count) QLX_HIP(hipMemcpy(dev, br.take(count * sizeof(T)), count * sizeof(T), hipMemcpyHostToDevice));
}

void learner_restore(snap::Reader& r, qlx_learner* L, snap::BlobReader& head, FrameIo* io) {
  hipStream_t s = L->stream;
  const uint32_t N = L->N;
  L->step_count = head.u64();
  L->vec_steps = head.u64();
  L->update_count = head.u64();
  L->stats_events = head.u64();
  L->seen_episodes = head.u64();
  const uint64_t log_len = head.u64();
  const uint8_t* log = head.take(log_len);
  L->last_log.assign(reinterpret_cast<const char*>(log), log_len);
  head.done();
  {   // env
    const std::vector<uint8_t> buf = r.small(snap::SEC_ENV);
    snap::BlobReader br(buf, snap::SEC_ENV);
    qlx_env* e = L->env;
    if (br.u32() != N) throw snap::FormatError{"snapshot: env section n_envs disagrees with the parameters"};
    e->id_offset = br.u32();
    e->seed = br.u64();
    e->hashing = br.u32() != 0;
    (void)br.u32();
    get_device(br, e->d_state.get(), N);
    get_device(br, e->d_ep_steps.get(), N);
    get_device(br, e->d_hash.get(), N);
    get_device(br, e->d_flags.get(), 4);
    br.done();
    frames_read(r, snap::SEC_ENV_FRAMES, FrameRing{e->d_obs, (uint64_t)N * kSlots, 0, (uint64_t)N * kSlots}, s, io);
  }
  replay_restore(r, L->rb, s, io);
  model_section_read(r, snap::SEC_MODEL_ONLINE, L->online);
  model_section_read(r, snap::SEC_MODEL_TARGET, L->target);
  {   // episode books
    const std::vector<uint8_t> buf = r.small(snap::SEC_BOOKS);
    snap::BlobReader br(buf, snap::SEC_BOOKS);
    const uint32_t hist_cap = (uint32_t)L->p.episode_reward_history_buffer_len;
    Book b{};
    b.episode_count = br.u64();
    b.running_reward = br.f32();
    b.hist_len = br.u32();
    b.hist_head = br.u32();
    if (br.u32() != hist_cap || b.hist_len > hist_cap || (b.hist_head >= hist_cap))
      throw snap::FormatError{"snapshot: episode reward history disagrees with the parameters"};
    QLX_HIP(hipMemcpy(L->d_book, &b, sizeof(Book), hipMemcpyHostToDevice));
    get_device(br, L->d_ep_reward.get(), N);
    const float* hist = reinterpret_cast<const float*>(br.take((uint64_t)b.hist_len * sizeof(float)));
    br.done();
    ring_from_host(L->d_hist.get(), hist, hist_cap, b.hist_head, b.hist_len);
  }
  if (L->per) {
    const std::vector<uint8_t> buf = r.small(snap::SEC_PER);
    snap::BlobReader br(buf, snap::SEC_PER);
    if (br.u64() != L->prio.cap) throw snap::FormatError{"snapshot: prioritized-replay capacity disagrees with the parameters"};
    get_device(br, L->prio.d_max.get(), 1);
    get_device(br, L->prio.leaves(), L->prio.cap);   // the inner nodes are rebuilt before every draw (per_launch_build)
    br.done();
  }
  if (L->ycache) {
    if (r.find(snap::SEC_MEMO)) {
      const std::vector<uint8_t> buf = r.small(snap::SEC_MEMO);
      snap::BlobReader br(buf, snap::SEC_MEMO);
      const uint64_t len = L->rb->len();
      if (br.u64() != len) throw snap::FormatError{"snapshot: target memo length disagrees with the replay"};
      const float* y = reinterpret_cast<const float*>(br.take(len * sizeof(float)));
      br.done();
      ring_from_host(L->d_ycache.get(), y, L->rb->cap, (L->rb->total - len) % L->rb->cap, len);
      L->ycache_version = L->target->version;
    } else {
      L->ycache_version = L->target->version - 1;   // no memo in the file: the next push rebuilds every live slot
    }
  }
  L->last_updates = 0;
  QLX_HIP(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

int32_t qlx_learner_save(qlx_learner* L, const char* path) {
  return guard([&] {
    QLX_CHECK(L && path, QLX_E_INVALID, "null argument");
    QLX_HIP(hipSetDevice(L->device));
    QLX_HIP(hipStreamSynchronize(L->stream));
    if (L->comm_stream) QLX_HIP(hipStreamSynchronize(L->comm_stream));
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = L->stream;
    const uint32_t N = L->N;
    FrameIo io;
    io.codec = snapshot_codec_from_env();
    snapshot_timing_begin(&io);
    uint64_t file_bytes = 0;
    io_guard([&] {
      snap::Writer w(path, QLX_SNAPSHOT_LEARNER);
      const EpisodeBooks books = L->books();
      const Book& book = books.book;
      {
        snap::Blob b;
        b.put(&L->p, sizeof(qlx_params));
        b.u32(L->p.qnet_precision);
        b.u32((uint32_t)L->rank);
        b.u64(L->step_count);
        b.u64(L->vec_steps);
        b.u64(L->update_count);
        b.u64(L->stats_events);
        b.u64(L->seen_episodes);
        b.u64(L->last_log.size());
        b.put(L->last_log.data(), L->last_log.size());
        w.small(snap::SEC_LEARNER, b.bytes.data(), b.bytes.size());
      }
      {
        const qlx_env* e = L->env;
        snap::Blob b;
        b.u32(N);
        b.u32(e->id_offset);
        b.u64(e->seed);
        b.u32(e->hashing ? 1 : 0);
        b.u32(0);
        put_device(b, e->d_state.get(), N);
        put_device(b, e->d_ep_steps.get(), N);
        put_device(b, e->d_hash.get(), N);
        put_device(b, e->d_flags.get(), 4);
        w.small(snap::SEC_ENV, b.bytes.data(), b.bytes.size());
        frames_write(w, snap::SEC_ENV_FRAMES, FrameRing{e->d_obs, (uint64_t)N * kSlots, 0, (uint64_t)N * kSlots}, s, &io);
      }
      replay_write(w, L->rb, s, &io);
      model_section_write(w, snap::SEC_MODEL_ONLINE, L->online);
      model_section_write(w, snap::SEC_MODEL_TARGET, L->target);
      {
        const uint32_t hist_cap = (uint32_t)L->p.episode_reward_history_buffer_len;
        snap::Blob b;
        b.u64(book.episode_count);
        b.f32(book.running_reward);
        b.u32(book.hist_len);
        b.u32(book.hist_head);
        b.u32(hist_cap);
        put_device(b, L->d_ep_reward.get(), N);
        // the entries in use, oldest first (the rest of the ring was never written)
        b.put(books.rewards.data(), books.rewards.size() * sizeof(float));
        w.small(snap::SEC_BOOKS, b.bytes.data(), b.bytes.size());
      }
      if (L->per) {
        snap::Blob b;
        b.u64(L->prio.cap);
        put_device(b, L->prio.d_max.get(), 1);
        put_device(b, L->prio.leaves(), L->prio.cap);
        w.small(snap::SEC_PER, b.bytes.data(), b.bytes.size());
      }
      if (L->ycache && L->ycache_version == L->target->version) {   // y (or v) of the live slots, oldest first
        const uint64_t len = L->rb->len();
        snap::Blob b;
        b.u64(len);
        if (len)
          ring_to_host(reinterpret_cast<float*>(b.grow(len * sizeof(float))), L->d_ycache.get(), L->rb->cap,
                       (L->rb->total - len) % L->rb->cap, len);
        w.small(snap::SEC_MEMO, b.bytes.data(), b.bytes.size());
      }
      qlx_snapshot_info info{};
      info.format_version = QLX_SNAPSHOT_VERSION;
      info.kind = QLX_SNAPSHOT_LEARNER;
      info.frame_codec = (uint32_t)io.codec;
      info.step_count = L->step_count;
      info.vec_steps = L->vec_steps;
      info.update_count = L->update_count;
      info.episode_count = book.episode_count;
      info.replay_len = L->rb->len();
      info.replay_total = L->rb->total;
      info.frames = io.frames;
      info.frame_bytes_raw = io.raw_bytes;
      info.frame_bytes_stored = io.stored_bytes;
      info.file_bytes = w.position() + sizeof(info);
      info.params = L->p;
      w.small(snap::SEC_INFO, &info, sizeof(info));
      file_bytes = w.finish();
    });
    snapshot_timing_report("learner_save", io, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), file_bytes);
  });
}

int32_t qlx_learner_load(const char* path, int32_t device, qlx_learner** out) {
  return guard([&] {
    QLX_CHECK(path && out, QLX_E_INVALID, "null argument");
    const auto t0 = std::chrono::steady_clock::now();
    FrameIo io;
    snapshot_timing_begin(&io);
    io_guard([&] {
      snap::Reader r(path, QLX_SNAPSHOT_LEARNER);
      const std::vector<uint8_t> buf = r.small(snap::SEC_LEARNER, 1u << 24);
      snap::BlobReader head(buf, snap::SEC_LEARNER);
      qlx_params p;
      head.get(&p, sizeof(p));
      if (head.u32() != p.qnet_precision || head.u32() != p.rank)
        throw snap::FormatError{"snapshot: learner section disagrees with its parameters"};
      qlx_learner* L = nullptr;
      const int32_t st = qlx_learner_create(&p, device, &L);
      QLX_CHECK(st == QLX_OK, st, qlx_last_error());
      try {
        learner_restore(r, L, head, &io);
      } catch (...) {
        qlx_learner_destroy(L);
        throw;
      }
      *out = L;
      snapshot_timing_report("learner_load", io, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                             r.header().file_bytes);
    });
  });
}

}  // extern "C"
