# Build of the MI355X engine (gfx950 only) and of its test infrastructure.
#   make lib      narwhal_amd/lib/libnwv.so   (product: HIP kernels + C ABI, include/nwv.h)
#   make oracle   oracle/build/libnwv_oracle.so (test infrastructure: CPU restatement)
#   make hostemu  tests/_build/libhostemu.so    (test infrastructure: device math on the host)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
BLS_SRC := narwhal_amd/csrc/nwv_bls.hip narwhal_amd/csrc/bls381.h narwhal_amd/csrc/bls_verify.h narwhal_amd/csrc/bls_group.h \
	narwhal_amd/csrc/bls381_consts.h narwhal_amd/csrc/bls381_iso.h narwhal_amd/csrc/bls_wave.h \
	narwhal_amd/csrc/bls_wave_prog.h narwhal_amd/csrc/bls_shard.h narwhal_amd/csrc/bls_msg_ring.h \
	narwhal_amd/csrc/bls_apk_ring.h narwhal_amd/csrc/bls_key_batch.h narwhal_amd/csrc/bls_apk_dense.h \
	include/nwv_bls.h
# headers that both engines' translation units include (they stay in CSRC)
BLS_SHARED := narwhal_amd/csrc/shard.h narwhal_amd/csrc/place.h narwhal_amd/csrc/lane_pool.h narwhal_amd/csrc/lane_stream.h
CSRC := $(filter-out $(BLS_SRC),$(wildcard narwhal_amd/csrc/*.h narwhal_amd/csrc/*.hip narwhal_amd/csrc/*.cpp)) \
	include/nwv.h include/nwv_types.h include/nwv_service.h include/nwv_digest_stream.h

all: lib oracle hostemu tools

lib: narwhal_amd/lib/libnwv.so
# nwv_types.cpp is plain host C++ (no kernels): built by g++ on its own, because mixing `-x c++`
# into the hipcc line makes hipcc drop --offload-arch (the code object silently falls back to gfx906)
narwhal_amd/lib/nwv_types.o: narwhal_amd/csrc/nwv_types.cpp include/nwv.h include/nwv_types.h include/nwv_bls.h
	@mkdir -p narwhal_amd/lib
	g++ -O2 -std=c++17 -fPIC -Wall -c -o $@ $<
narwhal_amd/lib/nwv_service.o: narwhal_amd/csrc/nwv_service.cpp include/nwv.h include/nwv_types.h include/nwv_service.h
	@mkdir -p narwhal_amd/lib
	g++ -O2 -std=c++17 -fPIC -Wall -c -o $@ $<
# the BLS12-381 engine is its own translation unit (compiled in parallel with the Ed25519 one)
narwhal_amd/lib/nwv_bls.o: $(BLS_SRC) $(BLS_SHARED) include/nwv.h
	@mkdir -p narwhal_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -c -o $@ narwhal_amd/csrc/nwv_bls.hip
narwhal_amd/lib/nwv_host.o: $(CSRC)
	@mkdir -p narwhal_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -c -o $@ narwhal_amd/csrc/nwv_host.hip
narwhal_amd/lib/libnwv.so: narwhal_amd/lib/nwv_host.o narwhal_amd/lib/nwv_bls.o narwhal_amd/lib/nwv_types.o \
		narwhal_amd/lib/nwv_service.o
	@mkdir -p narwhal_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -o $@ narwhal_amd/lib/nwv_host.o narwhal_amd/lib/nwv_bls.o \
		narwhal_amd/lib/nwv_types.o narwhal_amd/lib/nwv_service.o -lpthread

oracle:
	$(MAKE) -C oracle

hostemu: tests/_build/libhostemu.so tests/_build/libsvcstub.so tests/_build/libblsemu.so tests/_build/libblsshard.so \
	tests/_build/libcombemu.so tests/_build/libfeseeded.so tests/_build/libtrimemu.so tests/_build/libfoldemu.so \
	tests/_build/libplace.so tests/_build/libkcalloc.so tests/_build/libgroupkeys.so tests/_build/libeachemu.so \
	tests/_build/libblswbemu.so tests/_build/libblsmsgring.so tests/_build/libblsmremu.so \
	tests/_build/libblsapkring.so tests/_build/libblsaremu.so tests/_build/libblskeybatch.so \
	tests/_build/libblskbemu.so tests/_build/libblsademu.so tests/_build/libblswvemu.so \
	tests/_build/libcombpassemu.so tests/_build/libtypedfusedemu.so \
	tests/_build/libtailrcemu.so tests/_build/liblanepool.so tests/_build/libdstream.so \
	tests/_build/libedplan.so
# the digest stream (digest_stream.h: chunk pool, hold-back rule, tick plan, pump, callbacks) over a stub
# device that runs the work records with blake2b.h's compression (tests/test_digest_stream_host.py)
tests/_build/libdstream.so: tests/hostemu/digest_stream_stub.cpp narwhal_amd/csrc/digest_stream.h \
		narwhal_amd/csrc/blake2b.h narwhal_amd/csrc/sha512.h narwhal_amd/csrc/fe25519.h
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 -g --offload-host-only -x hip -fPIC -shared -pthread -o $@ tests/hostemu/digest_stream_stub.cpp
# the wave interpreter one program at a time with its limb bounds evaluated (BLS_BOUNDS_CHECK;
# tests/test_bls_wave_vectors_hostemu.py)
tests/_build/libblswvemu.so: tests/hostemu/bls_wave_vectors_hostemu.cpp $(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O2 --offload-host-only -x hip -DBLS_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/bls_wave_vectors_hostemu.cpp
# the key-transposed batch check's host pass (bls_key_batch.h) with no HIP (tests/test_bls_key_batch_host.py)
tests/_build/libblskeybatch.so: tests/hostemu/bls_key_batch_stub.cpp narwhal_amd/csrc/bls_key_batch.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -o $@ tests/hostemu/bls_key_batch_stub.cpp
# the key-transposed batch check's stages on the host (tests/test_bls_key_batch_hostemu.py)
tests/_build/libblskbemu.so: tests/hostemu/bls_key_batch_hostemu.cpp tests/hostemu/bls_wave_batch_hostemu.cpp \
		$(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O2 --offload-host-only -x hip -fPIC -shared -o $@ tests/hostemu/bls_key_batch_hostemu.cpp
# the dense key-sum stage's per-group arithmetic and routing on the host (tests/test_bls_apk_dense_hostemu.py)
tests/_build/libblsademu.so: tests/hostemu/bls_apk_dense_hostemu.cpp $(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O2 --offload-host-only -x hip -fPIC -shared -o $@ tests/hostemu/bls_apk_dense_hostemu.cpp
# the message ring's bookkeeping (bls_msg_ring.h) with no HIP (tests/test_bls_msg_ring_host.py)
tests/_build/libblsmsgring.so: tests/hostemu/bls_msg_ring_stub.cpp narwhal_amd/csrc/bls_msg_ring.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/bls_msg_ring_stub.cpp
# the hash role of a call that uses the message ring (k_blsw_pre_r's item function) on the host
# (tests/test_bls_msg_ring_hostemu.py)
tests/_build/libblsmremu.so: tests/hostemu/bls_msg_ring_hostemu.cpp $(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O2 --offload-host-only -x hip -fPIC -shared -o $@ tests/hostemu/bls_msg_ring_hostemu.cpp
# the aggregate-key ring's bookkeeping (bls_apk_ring.h) with no HIP (tests/test_bls_apk_ring_host.py)
tests/_build/libblsapkring.so: tests/hostemu/bls_apk_ring_stub.cpp narwhal_amd/csrc/bls_apk_ring.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/bls_apk_ring_stub.cpp
# the fill of an aggregate-key ring slot (k_blsw_apk_fill's item function) and a hit item's pairing
# check on the host (tests/test_bls_apk_ring_hostemu.py)
tests/_build/libblsaremu.so: tests/hostemu/bls_apk_ring_hostemu.cpp $(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O2 --offload-host-only -x hip -fPIC -shared -o $@ tests/hostemu/bls_apk_ring_hostemu.cpp
# the trait surface's grouping of a batch's keys (group_keys.h) with no HIP (tests/test_group_keys_host.py)
tests/_build/libgroupkeys.so: tests/hostemu/group_keys_stub.cpp narwhal_amd/csrc/group_keys.h
	@mkdir -p tests/_build
	g++ -O2 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/group_keys_stub.cpp
# the key cache's slot / table bookkeeping and its hold (keycache_alloc.h) with no HIP
# (tests/test_keycache_alloc_host.py)
tests/_build/libkcalloc.so: tests/hostemu/keycache_alloc_stub.cpp narwhal_amd/csrc/keycache_alloc.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/keycache_alloc_stub.cpp
# the placement policy of a multi-device context (place.h) with no HIP (tests/test_place_host.py)
tests/_build/libplace.so: tests/hostemu/place_stub.cpp narwhal_amd/csrc/place.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/place_stub.cpp
# the Ed25519 path choice (ed_plan.h) with no HIP (tests/test_ed_plan_host.py)
tests/_build/libedplan.so: tests/hostemu/ed_plan_stub.cpp narwhal_amd/csrc/ed_plan.h include/nwv.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -o $@ tests/hostemu/ed_plan_stub.cpp
# the lane pools' lease rule (lane_pool.h) with no HIP (tests/test_lane_pool_host.py)
tests/_build/liblanepool.so: tests/hostemu/lane_pool_stub.cpp narwhal_amd/csrc/lane_pool.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/lane_pool_stub.cpp
# the BLS and Ed25519 calls' split over a multi-device context (bls_shard.h, shard.h) with stub per-device work
tests/_build/libblsshard.so: tests/hostemu/bls_shard_stub.cpp narwhal_amd/csrc/bls_shard.h narwhal_amd/csrc/shard.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/bls_shard_stub.cpp
# the gfx950 BLS12-381 code compiled for the host (tests/test_bls_hostemu.py)
tests/_build/libblsemu.so: tests/hostemu/bls_hostemu.cpp $(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O2 --offload-host-only -x hip -fPIC -shared -o $@ tests/hostemu/bls_hostemu.cpp
# the wave engine's batch check (one final exponentiation a group) on the host
# (tests/test_bls_wave_batch_hostemu.py)
tests/_build/libblswbemu.so: tests/hostemu/bls_wave_batch_hostemu.cpp $(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O2 --offload-host-only -x hip -fPIC -shared -o $@ tests/hostemu/bls_wave_batch_hostemu.cpp
# the same build under AddressSanitizer + UndefinedBehaviorSanitizer (host code only):
#   make blsemu-asan && tools/run_blsemu_asan.sh
tests/_build/libblsemu_asan.so: tests/hostemu/bls_hostemu.cpp $(BLS_SRC) $(BLS_SHARED)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 -g --offload-host-only -x hip -fPIC -shared -fno-omit-frame-pointer \
		-fno-gpu-sanitize -fsanitize=address,undefined -fno-sanitize-recover=all -shared-libsan \
		-o $@ tests/hostemu/bls_hostemu.cpp
blsemu-asan: tests/_build/libblsemu_asan.so
# the batching service's host logic over a stubbed engine (tests/test_service_host.py)
tests/_build/libsvcstub.so: tests/hostemu/service_stub.cpp narwhal_amd/csrc/nwv_service.cpp include/nwv_service.h
	@mkdir -p tests/_build
	g++ -O1 -g -std=c++17 -fPIC -shared -pthread -o $@ tests/hostemu/service_stub.cpp narwhal_amd/csrc/nwv_service.cpp
tests/_build/libhostemu.so: tests/hostemu/hostemu.cpp $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/hostemu.cpp
# the comb kernel's per-signature arithmetic on the host (tests/test_comb_hostemu.py)
tests/_build/libcombemu.so: tests/hostemu/comb_hostemu.cpp $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/comb_hostemu.cpp
# the comb pass kernel's per-signature arithmetic on the host (tests/test_comb_pass_hostemu.py)
tests/_build/libcombpassemu.so: tests/hostemu/comb_pass_hostemu.cpp tests/hostemu/comb_hostemu.cpp $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/comb_pass_hostemu.cpp
# the one-launch typed path on the host: the one-block BLAKE2b, the fused kernels' typed messages on the
# comb emulation, and nwv_types.cpp over a stub engine that records its plan (tests/test_typed_fused_hostemu.py)
tests/_build/libtypedfusedemu.so: tests/hostemu/typed_fused_hostemu.cpp tests/hostemu/comb_hostemu.cpp \
		narwhal_amd/csrc/nwv_types.cpp include/nwv_types.h include/nwv_bls.h $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ \
		tests/hostemu/typed_fused_hostemu.cpp narwhal_amd/csrc/nwv_types.cpp
# the row kernel's per-signature arithmetic on the host (tests/test_each_row_hostemu.py)
tests/_build/libeachemu.so: tests/hostemu/each_row_hostemu.cpp $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/each_row_hostemu.cpp
# fe25519.h's multiply and squaring in every column-sum form, column sums asserted below 2^63
# (tests/test_fe_seeded_hostemu.py)
tests/_build/libfeseeded.so: tests/hostemu/fe_seeded_hostemu.cpp narwhal_amd/csrc/fe25519.h
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/fe_seeded_hostemu.cpp
# the seeded bucket accumulator, fe_sq's operand split, ge_p1p1_to_p3's operand roles and the
# prefixed SHA-512 on the host (tests/test_trim_hostemu.py)
tests/_build/libtrimemu.so: tests/hostemu/trim_hostemu.cpp $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/trim_hostemu.cpp
# the tail's chunk planes by rows and columns on the host (tests/test_tail_rc_hostemu.py)
tests/_build/libtailrcemu.so: tests/hostemu/tail_rc_hostemu.cpp $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/tail_rc_hostemu.cpp
# the reduction mod l by folding, the unreduced sums of z s, the in-order digit recoding and the
# decompression with its stash on the host (tests/test_fold_hostemu.py)
tests/_build/libfoldemu.so: tests/hostemu/fold_hostemu.cpp $(CSRC)
	@mkdir -p tests/_build
	$(HIPCC) -std=c++17 -O1 --offload-host-only -x hip -DNWV_BOUNDS_CHECK -fPIC -shared -o $@ tests/hostemu/fold_hostemu.cpp

tools: tools/ubench_valu tools/ubench_field tools/ubench_wave tools/ubench_row tools/ubench_prep tools/libsvcbench.so \
	tools/fe_vectors tools/bls_wave_vectors
# the device's wave interpreter, fp_inv_wave and the F == 1 verdicts on slot images from a file
# (tests/test_gpu_bls_wave_vectors.py)
tools/bls_wave_vectors: tools/bls_wave_vectors.hip $(BLS_SRC)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<
# the device's fe_mul / fe_sq / fe_sqn on limb vectors from a file (tests/test_gpu_fe_seeded.py)
tools/fe_vectors: tools/fe_vectors.hip narwhal_amd/csrc/fe25519.h
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<
# native drivers of the C5 service leg (bench tooling): the service and the Core drain timed from C++ threads
tools/libsvcbench.so: tools/svcbench.cpp narwhal_amd/lib/libnwv.so include/nwv.h include/nwv_types.h include/nwv_service.h
	g++ -O2 -std=c++17 -fPIC -shared -pthread -Wall -o $@ $< -Lnarwhal_amd/lib -lnwv -Wl,-rpath,'$$ORIGIN/../narwhal_amd/lib'
tools/ubench_valu: tools/ubench_valu.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
tools/ubench_field: tools/ubench_field.hip narwhal_amd/csrc/fe25519.h
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<
tools/ubench_wave: tools/ubench_wave.hip $(BLS_SRC)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $<
tools/ubench_row: tools/ubench_row.hip narwhal_amd/csrc/fe_row.h narwhal_amd/csrc/msm.h
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Wno-unused-value -o $@ $<
tools/ubench_prep: tools/ubench_prep.hip $(CSRC)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Wno-unused-value -o $@ $<

clean:
	rm -rf narwhal_amd/lib tests/_build
	$(MAKE) -C oracle clean

.PHONY: blsemu-asan all lib oracle hostemu tools clean
