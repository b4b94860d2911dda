// Host-side address check of the fp32 GEMM policies (qnet32_kernels.h): every operand load and epilogue store a
// launch of qnet32.hip would issue is replayed on the CPU against host buffers of exactly the device workspace
// sizes, under AddressSanitizer, through the code the device runs: a policy builds its streams per thread, writes
// their LDS tables and issues every slab's buffer loads (host stand-ins for the descriptor and the loads, which also
// check the descriptor's byte count against the host buffer).  Dev tool (no GPU needed):
//   hipcc --offload-host-only -x hip -I q-learning_amd/csrc -I include -fsanitize=address -g -O1 \
//         scripts/q32_host_check.hip -o /tmp/q32_host_check && /tmp/q32_host_check 32 128
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host, device))
#define QLX_Q32_POLICIES_ONLY
#include "qnet32_kernels.h"

#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

using namespace qlx;
using namespace qlx::q32;

static Grid grid(int M, int BM, int N, int BN, int nz) { return Grid{(M + BM - 1) / BM, (N + BN - 1) / BN, nz}; }

static long checks = 0;

void HostLoads::bad_load(uint32_t voff, uint32_t soff, uint32_t bytes) const {
  fprintf(stderr, "%s: block %d slab %d thread %d: buffer load at lane offset %u + scalar offset %u is neither inside the descriptor's "
                  "%u bytes nor a load the stream put past them (lane offset >= %u)\n", policy, block, slab, tid, voff, soff, bytes, past);
  exit(1);
}
// (a launch builds the same few descriptors in every thread: each distinct one is looked up in the shadow memory once)
void HostLoads::check_rsrc(const char* base, uint32_t bytes) const {
  static std::set<std::pair<const char*, uint32_t>> held;
  if (!held.insert({base, bytes}).second || !__asan_region_is_poisoned(const_cast<char*>(base), bytes)) return;
  fprintf(stderr, "%s: block %d thread %d: a descriptor of %u bytes reaches past its host buffer\n", policy, block, tid, bytes);
  exit(1);
}

// past: the smallest lane offset at which the launch's streams ask for zeros
template <class P>
static void replay(const P& p, const char* name, uint32_t past = kOob) {
  using OA = Opnd<P::BM, P::A_KMAJ>;
  using OB = Opnd<P::BN, P::B_KMAJ>;
  constexpr int T = P::WM * P::WN * 64;   // threads of one K group
  constexpr int TM = P::BM / (P::WM * 16), TN = P::BN / (P::WN * 16);
  host_loads = HostLoads{name, 0, 0, 0, past, 0, 0};
  float* lds = static_cast<float*>(std::malloc(gemm_lds_bytes<P>()));   // (the streams' tables: exact size)
  for (int lb = 0; lb < p.g.blocks(); ++lb) {
    int tm, tn, z;
    p.decode(lb, tm, tn, z);
    const int row0 = tm * P::BM, col0 = tn * P::BN;
    if constexpr (HasActive<P>::value) {
      if (!p.active(z, row0)) continue;
    }
    host_loads.block = lb;
    // gemm_body: per K group the streams of its T threads, their tables, then the slabs
    using St = typename P::Streams;
    constexpr int G = KSplitOf<P>::value, GROUP_LDS = 2 * (OA::FLOATS + OB::FLOATS);
    const int ns = p.nslabs(z) / G;
    static std::vector<St> st(T);
    for (int tid = 0; tid < T; ++tid) {   // (the same in every group)
      host_loads.tid = tid;
      st[tid] = p.streams(z, row0, col0, tid);
    }
    for (int kg = 0; kg < G; ++kg) {
      if constexpr (HasPrepare<St>::value)
        for (int tid = 0; tid < T; ++tid) st[tid].prepare(lds + kg * GROUP_LDS, ns);
      for (int s = 0; s < ns; ++s) {
        host_loads.slab = kg * ns + s;
        for (int tid = 0; tid < T; ++tid) {
          host_loads.tid = tid;
          typename St::Regs x;
          st[tid].load(kg * ns + s, x);
        }
      }
    }
    for (int wave = 0; wave < T / 64; ++wave) {
      const int wm = wave % P::WM, wn = wave / P::WM;
      for (int i = 0; i < TM; ++i)
        for (int j = 0; j < TN; ++j)
          for (int lane = 0; lane < 64; ++lane) {
            const int row = row0 + (wm * TM + i) * 16 + (lane >> 4) * 4, col = col0 + (wn * TN + j) * 16 + (lane & 15);
            if constexpr (HasEpiPre<P>::value) {
              const auto m = p.epi_pre(z, row, col);
              p.epi_post(z, row, col, zero4(), m);
            } else {
              p.epi(z, row, col, zero4());
            }
          }
    }
    if constexpr (P::BIAS) {
      if (tm == 0)
        for (int t = 0; t < P::BN; ++t) p.epi_bias(z, col0 + t, 0.0f);
    }
  }
  std::free(lds);
  printf("%-24s blocks %6d buffer loads %10ld in range %9ld zero-filled ok\n", name, p.g.blocks(), host_loads.in_range, host_loads.zero_filled);
  checks += host_loads.in_range + host_loads.zero_filled;
}

template <class T>
static T* buf(size_t n) { return static_cast<T*>(std::calloc(n, sizeof(T))); }

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 32;       // training batch
  const int n = argc > 2 ? atoi(argv[2]) : B;        // forward batch (target pass)
  const int C = n;                                    // forward chunk = whole pass here
  // params in Keras layouts, exact sizes
  float* w0 = buf<float>(8 * 8 * 4 * 32); float* b0 = buf<float>(32);
  float* w1 = buf<float>(4 * 4 * 32 * 64); float* b1 = buf<float>(64);
  float* w2 = buf<float>(3 * 3 * 64 * 64); float* b2 = buf<float>(64);
  float* w3 = buf<float>(3136 * 512); float* b3 = buf<float>(512);
  // frames: every table entry its own 7,056-byte allocation
  const int F = std::max(B, n);
  std::vector<const uint8_t*> table(F * 4);
  for (size_t i = 0; i < table.size(); ++i)   // every 5th entry null: a ring slot before an episode's first frame
    table[i] = i % 5 == 3 ? nullptr : buf<uint8_t>(kFramePix);
  const uint8_t* const* tab = table.data();
  // a1, a2, a3 and the constant rows (relu(b0) [32], c2 [64], c3 [64]) in one allocation in f32_workspace's order, as on the
  // device: the list forward's one descriptor spans `in` and cx (PConvFwdL::streams).  The gaps between them are poisoned.
  const size_t asz[4] = {(size_t)C * 12800 * 4, (size_t)C * 5184 * 4, (size_t)C * 3136 * 4, 160 * 4};
  size_t aoff[5] = {0};
  for (int i = 0; i < 4; ++i) aoff[i + 1] = (aoff[i] + asz[i] + 255) / 256 * 256 + 256;
  char* arena = buf<char>(aoff[4]);
  for (int i = 0; i < 4; ++i) ASAN_POISON_MEMORY_REGION(arena + aoff[i] + asz[i], aoff[i + 1] - aoff[i] - asz[i]);
  float* a1 = (float*)(arena + aoff[0]); float* a2 = (float*)(arena + aoff[1]); float* a3 = (float*)(arena + aoff[2]);
  float* cx = (float*)(arena + aoff[3]); float* c2 = cx + 32; float* c3 = cx + 96;
  float* a4 = buf<float>((size_t)n * 512);
  // forward over n, every launch form of f32_forward.  Dense frames (no row lists): the 64 x 64 tiles of the chunk-size
  // pass, the training batch's 64 x 32 tiles and its balanced grid's 16-row remainder tiles (RowShift)
  replay(PConv2Fwd{grid(n * 81, 64, 64, 64, 1), a1, w1, b1, a2, n * 81}, "conv2_fwd");
  replay(PConv3Fwd{grid(n * 49, 64, 64, 64, 1), a2, w2, b2, a3, n * 49}, "conv3_fwd");
  replay(PConv2FwdS{grid(n * 81, 64, 64, 32, 1), a1, w1, b1, a2, n * 81}, "conv2_fwd S");
  replay(PConv3FwdS{grid(n * 49, 64, 64, 32, 1), a2, w2, b2, a3, n * 49}, "conv3_fwd S");
  {  // the last three whole tiles' rows and the rows after them as 16 x 64 tiles
    const int M2 = n * 81, M3 = n * 49, whole2 = std::max(0, M2 / 64 - 3), whole3 = std::max(0, M3 / 64 - 3);
    replay(PConv2FwdR{{Grid{(M2 - whole2 * 64 + 15) / 16, 1, 1}, a1, w1, b1, a2, M2}, whole2 * 4}, "conv2_fwd R");
    replay(PConv3FwdR{{Grid{(M3 - whole3 * 64 + 15) / 16, 1, 1}, a2, w2, b2, a3, M3}, whole3 * 4}, "conv3_fwd R");
  }
  {  // row-list forwards (background rows): per region a permutation of the rows, 2 / 3 of them non-background (or all),
     // conv3 entries carrying constant-tap masks; the constant-row tiles
    const int G = std::min(n, 512), per_slot = ((G + kListSlots - 1) / kListSlots) * ((n + G - 1) / G);
    const int cap2 = per_slot * 81, cap3 = per_slot * 49;
    int* rl2 = buf<int>((size_t)kListSlots * cap2);
    int* rl3 = buf<int>((size_t)kListSlots * cap3);
    for (int i = 0; i < kListSlots * cap2; ++i) rl2[i] = (int)(((long)i * 7919) % (n * 81));
    for (int i = 0; i < kListSlots * cap3; ++i) rl3[i] = (int)(((long)i * 7919) % (n * 49)) | ((i * 37) % 511) << 20;
    unsigned long long* cnt = buf<unsigned long long>(2 * kListSlots * kCntStride);
    for (int full = 0; full < 2; ++full) {
      for (int x = 0; x < kListSlots; ++x) {
        const unsigned long long k2 = full ? cap2 : cap2 * 2 / 3, k3 = full ? cap3 : cap3 * 2 / 3;
        cnt[(x * 2) * kCntStride] = k2 << 32 | (cap2 - k2);
        cnt[(x * 2 + 1) * kCntStride] = k3 << 32 | (cap3 - k3);
      }
      auto lg = [&](int cap, int BM, int BN) { return Grid{1 + kListSlots * ((cap + BM - 1) / BM), 64 / BN, 1}; };
      // conv2: one tile shape, the epilogue's list entries batched (chunk-size pass) or row by row (training batch)
      PConv2FwdL<64, 64, 2, 2> p2{lg(cap2, 64, 64), a1, w1, b1, a2, rl2, cap2, cnt, cx};
      replay(p2, "conv2_fwd L big");
      p2.pre_batched = false;
      replay(p2, "conv2_fwd L");
      replay(PConv3FwdL<64, 64, 2, 2>{lg(cap3, 64, 64), a2, w2, b2, a3, rl3, cap3, cnt + kCntStride, c2}, "conv3_fwd L big");
      replay(PConv3FwdL<32, 64, 2, 2>{lg(cap3, 32, 64), a2, w2, b2, a3, rl3, cap3, cnt + kCntStride, c2}, "conv3_fwd L");
    }
    // (ConstRows' two tiles: a descriptor over the constant input row alone, inside the constant rows' own region)
    replay(ConstRows::PA{cx, w1, b1, c2}, "const row c2");
    replay(ConstRows::PB{c2, w2, b2, c3}, "const row c3");
  }
  replay(PFc1FwdB{grid(n, PFc1FwdB::BM, 512, PFc1FwdB::BN, 1), a3, w3, b3, a4, n}, "fc1_fwd B");
  replay(PFc1FwdS{grid(n, PFc1FwdS::BM, 512, PFc1FwdS::BN, 1), a3, w3, b3, a4, n}, "fc1_fwd S");
  // backward over B (activations of a B-sample forward), every launch form of f32_backward_dense / f32_backward_conv; the
  // background buffers are those of the smallest workspace (need_ld = B rounded up to 64)
  float* dz1 = buf<float>((size_t)B * 12800); float* dz2 = buf<float>((size_t)B * 5184);
  float* dz3 = buf<float>((size_t)B * 3136); float* dz4 = buf<float>((size_t)B * 512);
  float* s2 = buf<float>((size_t)((B + kSC2 - 1) / kSC2) * 513 * 64);
  float* s3 = buf<float>((size_t)((B + kSC3 - 1) / kSC3) * 577 * 64);
  float* gw3 = buf<float>(3136 * 512); float* gb3 = buf<float>(512);
  const int z3 = (B + kSC3 - 1) / kSC3, z2 = (B + kSC2 - 1) / kSC2;
  const int need_ld = (B + 63) / 64 * 64;
  // non-background row bits of a layer's P rows per sample: a varying share (all, none, every k-th)
  auto row_bits = [&](int P) {
    uint32_t* rows = buf<uint32_t>((size_t)B * 4);
    for (int b = 0; b < B; ++b)
      for (int p = 0; p < P; ++p)
        if (b % 5 == 0 || (b % 5 != 1 && (p * 7 + b) % (2 + b % 3) == 0)) rows[(size_t)b * 4 + p / 32] |= 1u << (p % 32);
    return rows;
  };
  replay(PFc1WgradS{grid(3136, PFc1WgradS::BM, 512, PFc1WgradS::BN, 1), a3, dz4, gw3, gb3, B}, "fc1_wgrad S");
  {
    PFc1DgradS Pd{grid(B, PFc1DgradS::BM, 3136, PFc1DgradS::BN, 1), dz4, w3, a3, dz3, B};
    replay(Pd, "fc1_dgrad S");
    Pd.pbg = buf<float>((size_t)(B + 15) / 16 * 49 * 64);
    Pd.bg = buf<uint8_t>((size_t)49 * need_ld);
    Pd.bg_ld = need_ld;
    replay(Pd, "fc1_dgrad S pbg");
  }
  // (compacted: rows past the kept ones read at what the table's all-ones entry decodes to)
  replay(PConv3Wgrad{grid(576, 64, 64, 64, z3), a2, dz3, s3, B, row_bits(49)}, "conv3_wgrad compacted", std::min(PConv3Wgrad::TA::PAST, PConv3Wgrad::TB::PAST));
  replay(PConv3WgradD{grid(576, 64, 64, 64, z3), a2, dz3, s3, B}, "conv3_wgrad dense");
  {
    PConv3DgradP Pd{Grid{(B + PConv3DgradP::BM - 1) / PConv3DgradP::BM, 1, 81}, dz3, w2, a2, dz2, B};
    replay(Pd, "conv3_dgrad px");
    Pd.pbg = buf<float>((size_t)(B + 15) / 16 * 81 * 64);
    Pd.bg2 = buf<uint8_t>((size_t)81 * need_ld);
    Pd.bg2_ld = need_ld;
    replay(Pd, "conv3_dgrad px pbg");
  }
  replay(PConv2Wgrad{grid(512, 64, 64, 64, z2), a1, dz2, s2, B, row_bits(81)}, "conv2_wgrad compacted", std::min(PConv2Wgrad::TA::PAST, PConv2Wgrad::TB::PAST));
  replay(PConv2WgradD{grid(512, 64, 64, 64, z2), a1, dz2, s2, B}, "conv2_wgrad dense");
  {  // conv1's bias partials always; the step bytes when the forward built row lists
    PConv2DgradP Pd{Grid{(B + 63) / 64, 2, 100}, dz2, w1, a1, dz1, B, buf<float>((size_t)(B + 15) / 16 * 400 * 32)};
    replay(Pd, "conv2_dgrad px pb");
    Pd.need = buf<uint8_t>((size_t)100 * need_ld);
    Pd.need_ld = need_ld;
    replay(Pd, "conv2_dgrad px pb need");
  }
  printf("B %d n %d: %ld operand loads replayed, all in bounds\n", B, n, checks);
  return 0;
}
