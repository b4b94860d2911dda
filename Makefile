# Build of libqlx.so (HIP for gfx950 + C++ host) and the CPU oracle (test infrastructure).
#   make            -> q-learning_amd/lib/libqlx.so + oracle/liboracle.so + oracle/cpu_baseline
#   make lib        -> product only
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := q-learning_amd
SRC := $(PKG)/csrc
OUT := $(PKG)/lib
JOBS ?= 8

HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-result \
            -I include -I $(SRC) -munsafe-fp-atomics
# physics/raster must round every a*b+c twice like the reference (Rust never fuses)
STRICT := -ffp-contract=off
LDFLAGS := -shared -L/opt/rocm/lib -lamdhip64 -lrccl -Wl,-rpath,/opt/rocm/lib

OBJS := $(OUT)/obj/common.o $(OUT)/obj/env_breakout.o $(OUT)/obj/replay.o $(OUT)/obj/model.o $(OUT)/obj/qnet_bf16.o $(OUT)/obj/qnet32.o $(OUT)/obj/learner.o \
        $(OUT)/obj/ballgame.o $(OUT)/obj/tf_bundle.o $(OUT)/obj/per.o $(OUT)/obj/stats.o $(OUT)/obj/evaluator.o \
        $(OUT)/obj/snapshot_format.o $(OUT)/obj/frame_codec.o $(OUT)/obj/learner_core.o $(OUT)/obj/learner_snapshot.o \
        $(OUT)/obj/metrics.o $(OUT)/obj/batch_dev.o $(OUT)/obj/model_dev.o $(OUT)/obj/head_wide.o $(OUT)/obj/dist_loss.o

HDRS := include/qlx.h $(wildcard $(SRC)/*.h)

all: lib oracle

lib: $(OUT)/libqlx.so

$(OUT)/obj:
	mkdir -p $@

$(OUT)/obj/common.o: $(SRC)/common.cpp $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OUT)/obj/env_breakout.o: $(SRC)/env_breakout.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

$(OUT)/obj/replay.o: $(SRC)/replay.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# device-tensor env / replay calls: its window arithmetic is replay_dev.h's, under replay.o's flags
$(OUT)/obj/batch_dev.o: $(SRC)/batch_dev.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# device-tensor Q-net calls: byte-moving and pointer-table kernels only, model.o's flags
$(OUT)/obj/model_dev.o: $(SRC)/model_dev.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# (bf16 Q-net on the default scheduler since round 5: 789K -> 797K env-steps/s against max-ILP, the slab reduction
# 11.4 -> 10.0 us)
$(OUT)/obj/qnet_bf16.o: $(SRC)/qnet_bf16.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the precision-independent model layer (its two staging kernels came out of the bf16 file: the same flags)
$(OUT)/obj/model.o: $(SRC)/model.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# fp32 Q-net: bit-exact against the oracle, so no contraction anywhere (every fma is an explicit fmaf / MFMA)
# Q-net objects: the backend's max-ILP scheduling strategy (measured at C3: fp32 195.5K -> 196.2K env-steps/s, every GEMM
# layer equal or faster; max-memory-clause 191.0K, iterative-ilp 196.6K; bf16 745.7K -> 749.3K)
Q32SCHED := -mllvm --amdgpu-sched-strategy=max-ilp
# fp32 Q-net: MFMA accumulators in VGPRs (the AGPR form rotated the pair GEMMs' accumulators through v_accvgpr moves every
# slab - VALU time the fp32 MFMAs cannot overlap; measured: conv2 / conv3 pairs 96.4 / 72.1 -> 95.9 / 71.2 us)
Q32VFORM := -mllvm -amdgpu-mfma-vgpr-form=1

$(OUT)/obj/qnet32.o: $(SRC)/qnet32.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(Q32SCHED) $(Q32VFORM) -c $< -o $@

# the wide output head: fmaf chains pinned bit for bit to the fp32 head's, so qnet32.o's flags
$(OUT)/obj/head_wide.o: $(SRC)/head_wide.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(Q32SCHED) $(Q32VFORM) -c $< -o $@

# distributional losses on the wide head: the quantile loss is separately rounded fp32 operations the tests restate bit
# for bit (metrics.o's flags); the fused select kernel shares the values' device functions and therefore this object
$(OUT)/obj/dist_loss.o: $(SRC)/dist_loss.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

$(OUT)/obj/learner.o: $(SRC)/learner.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

# the environment-independent learner core (its two kernels came out of learner.hip: the same flags; the f32 running-reward
# sum is compared bit for bit with the oracle) and the learner's save / load
$(OUT)/obj/learner_core.o: $(SRC)/learner_core.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

$(OUT)/obj/learner_snapshot.o: $(SRC)/learner_snapshot.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

# per-update training metrics: its td = |q_a - y| and action gaps are single fp32 roundings the tests restate bit for bit
# (learner.o's flags)
$(OUT)/obj/metrics.o: $(SRC)/metrics.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

# policy evaluation: fp32 sums compared bit for bit with the oracle restatement, like the learner's books
$(OUT)/obj/evaluator.o: $(SRC)/evaluator.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

$(OUT)/obj/tf_bundle.o: $(SRC)/tf_bundle.cpp $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# BallGame env step is restated like the reference's f32 rewards (no FMA-sensitive math); the net is fp32 SIMT
$(OUT)/obj/ballgame.o: $(SRC)/ballgame.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# sum-tree descent and IS weights are compared bit-for-bit with the oracle: no contraction
$(OUT)/obj/per.o: $(SRC)/per.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

$(OUT)/obj/stats.o: $(SRC)/stats.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@

# snapshots: the container and the host reference of the frame codec (host only, no HIP call), and the codec's kernels
$(OUT)/obj/snapshot_format.o: $(SRC)/snapshot_format.cpp $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OUT)/obj/frame_codec.o: $(SRC)/frame_codec.hip $(HDRS) | $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OUT)/libqlx.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) $(OBJS) $(LDFLAGS) -o $@

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(OUT) && $(MAKE) -C oracle clean

.PHONY: all lib oracle clean
