// Host-side check of DeviceBuffer / PinnedBuffer (device_memory.h): the four allocation functions are defined here
// over malloc / free with a count of live allocations and a countdown that makes the k-th allocation throw
// QLX_E_OOM, so ownership, the failed-allocation paths and unwinding run on the CPU under AddressSanitizer and
// UBSan.  Exits non-zero at the first failed check.  Dev tool (no GPU needed):
//   hipcc --offload-host-only -x hip -I q-learning_amd/csrc -I include -fsanitize=address,undefined -g -O1 \
//         scripts/devmem_host_check.hip -o /tmp/devmem_host_check && /tmp/devmem_host_check
#include "qlx_internal.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

using namespace qlx;

static long live = 0;        // allocations not yet freed
static long fail_in = 0;     // > 0: the fail_in-th allocation from now throws

static void* counted_alloc(size_t bytes) {
  if (fail_in > 0 && --fail_in == 0) throw Error{QLX_E_OOM, "allocation of " + std::to_string(bytes) + " bytes refused"};
  ++live;
  return std::malloc(bytes);
}
static void counted_free(void* p) {
  --live;
  std::free(p);
}

namespace qlx {
void* device_alloc(size_t bytes) { return counted_alloc(bytes); }
void device_free(void* p) noexcept { counted_free(p); }
void* pinned_alloc(size_t bytes) { return counted_alloc(bytes); }
void pinned_free(void* p) noexcept { counted_free(p); }
}  // namespace qlx

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

template <class F>
static bool throws_oom(F&& f) {
  try {
    f();
  } catch (const Error& e) {
    return e.code == QLX_E_OOM;
  }
  return false;
}

struct Four {   // the ycache_reserve shape: four buffers grown one after the other
  DeviceBuffer<const uint8_t*> tab;
  DeviceBuffer<float> rew, tmp;
  DeviceBuffer<uint8_t> done;
  void reserve(size_t n) {
    tab.reserve(n * 4);
    rew.reserve(n);
    done.reserve(n);
    tmp.reserve(n);
  }
};

template <template <class> class Buf>
static void check_buffer() {
  {  // alloc, element access through the pointer conversion, destructor
    Buf<uint32_t> a;
    CHECK(!a && a.get() == nullptr && a.size() == 0 && a.bytes() == 0);
    a.alloc(7);
    CHECK(a && a.size() == 7 && a.bytes() == 28 && live == 1);
    uint32_t* p = a;
    for (int i = 0; i < 7; ++i) p[i] = i;
    CHECK(a.get() == p && a[6] == 6);
    // move construction and move assignment: the source is empty, nothing is allocated or freed
    Buf<uint32_t> b(std::move(a));
    CHECK(!a && a.size() == 0 && b.get() == p && b.size() == 7 && live == 1);
    Buf<uint32_t> c;
    c = std::move(b);
    CHECK(!b && b.size() == 0 && c.get() == p && c.size() == 7 && live == 1);
    Buf<uint32_t> d(3);   // move assignment onto a full buffer frees what it held
    CHECK(live == 2);
    d = std::move(c);
    CHECK(!c && d.get() == p && d.size() == 7 && live == 1);
  }
  CHECK(live == 0);
  {  // release
    Buf<float> a(5);
    CHECK(live == 1);
    a.release();
    CHECK(!a && a.size() == 0 && live == 0);
    a.release();
    CHECK(live == 0);
  }
  CHECK(live == 0);
  {  // reserve below and at the current size does not allocate; above it regrows
    Buf<float> a(16);
    float* p = a;
    fail_in = 1;   // any allocation would throw
    a.reserve(8);
    a.reserve(16);
    CHECK(a.get() == p && a.size() == 16 && live == 1 && fail_in == 1);
    fail_in = 0;
    a.reserve(17);
    CHECK(a.size() == 17 && live == 1);
    a.reset(4);   // reset shrinks too
    CHECK(a.size() == 4 && live == 1);
  }
  CHECK(live == 0);
  {  // reset / reserve with the allocation failing: empty, one allocation fewer, nothing left for the destructor
    Buf<float> a(16), b(16);
    CHECK(live == 2);
    fail_in = 1;
    CHECK(throws_oom([&] { a.reset(32); }));
    CHECK(!a && a.get() == nullptr && a.size() == 0 && a.bytes() == 0 && live == 1);
    fail_in = 1;
    CHECK(throws_oom([&] { b.reserve(32); }));
    CHECK(!b && b.size() == 0 && live == 0);
    a.reserve(2);   // usable again
    CHECK(a.size() == 2 && live == 1);
    a.release();
    fail_in = 1;    // alloc on an empty buffer failing
    CHECK(throws_oom([&] { a.alloc(2); }));
    CHECK(!a && a.size() == 0 && live == 0);
  }
  CHECK(live == 0);
  {  // zero-length alloc: empty, no call
    Buf<uint8_t> a;
    fail_in = 1;
    a.alloc(0);
    Buf<uint8_t> b(0);
    a.reset(0);
    a.reserve(0);
    CHECK(!a && !b && a.size() == 0 && live == 0 && fail_in == 1);
    fail_in = 0;
  }
  CHECK(live == 0);
}

int main() {
  check_buffer<DeviceBuffer>();
  check_buffer<PinnedBuffer>();
  // a struct of four buffers built in a try with the third allocation failing: nothing is left after unwinding
  CHECK(throws_oom([] {
    Four f;
    fail_in = 3;
    f.reserve(64);
  }));
  CHECK(live == 0);
  {  // the same as a regrow of a live object: the failed buffer is empty, the rest consistent, and a retry repairs it
    Four f;
    f.reserve(8);
    CHECK(live == 4);
    fail_in = 3;
    CHECK(throws_oom([&] { f.reserve(64); }));
    CHECK(f.tab.size() == 256 && f.rew.size() == 64 && !f.done && f.done.size() == 0 && f.tmp.size() == 8 && live == 3);
    f.reserve(8);
    CHECK(f.done.size() == 8 && live == 4);
    f.reserve(64);
    CHECK(f.done.size() == 64 && f.tmp.size() == 64 && live == 4);
  }
  CHECK(live == 0);
  printf("ok\n");
  return 0;
}
