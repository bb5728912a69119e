# Builds the in-tree native library (gfx950 only) and the CPU parity oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-result
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter
HDR = include/jsplace.h include/jsplace_bench.h include/jsk_host.h jobset_amd/csrc/jsp_internal.h jobset_amd/csrc/jsp_walk.h jobset_amd/csrc/jsp_multi.h jobset_amd/csrc/jsp_lines.h jobset_amd/csrc/jsp_wait.h jobset_amd/csrc/jsp_clock.h jobset_amd/csrc/jsp_leased_metrics.h jobset_amd/csrc/jsp_select.h
HOST_SRC = $(wildcard jobset_amd/csrc/host/*.cc)
HOST_HDR = $(wildcard jobset_amd/csrc/host/*.h)
HOST_OBJ = $(patsubst jobset_amd/csrc/host/%.cc,build/host_%.o,$(HOST_SRC))
LIB = jobset_amd/libjsplace.so
OBJ = build/jsp_kernels.o build/jsp_engine.o build/jsp_walk.o build/jsp_multi.o $(HOST_OBJ)

all: $(LIB) oracle

# -ffinite-math-only: the kernels' only floating point is the tally's f64
# capacity minimum (finite, non-negative): v_min_f64 without the NaN-quieting
# v_max_f64 the IEEE minNum semantics would put before each operand
KFLAGS = -ffinite-math-only
build/jsp_kernels.o: jobset_amd/csrc/jsp_kernels.hip jobset_amd/csrc/jsp_stamps.h $(HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) -c -o $@ $<

build/jsp_engine.o: jobset_amd/csrc/jsp_engine.cc jobset_amd/csrc/jsp_walk.h $(HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -x hip -c -o $@ $<

build/jsp_walk.o: jobset_amd/csrc/jsp_walk.cc jobset_amd/csrc/jsp_walk.h $(HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -x hip -c -o $@ $<

build/jsp_multi.o: jobset_amd/csrc/jsp_multi.cc jobset_amd/csrc/jsp_multi.h $(HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -x hip -c -o $@ $<

build/host_%.o: jobset_amd/csrc/host/%.cc $(HOST_HDR) $(HDR)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -c -o $@ $<

$(LIB): $(OBJ)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJ) -ldl

oracle:
	$(MAKE) -s -C oracle

# The one diagnostic build: the kernels with in-kernel phase stamps
# (jsp_stamps.h, read by tools/stamps.py) linked with the product's other
# objects; a tool loads it through JSP_LIB_PATH. Never the product library.
diag: tools/bin/diag/libjsplace.so tools/bin/dispatch_probe tools/bin/stream_ceiling
tools/bin/diag/libjsplace.so: jobset_amd/csrc/jsp_kernels.hip jobset_amd/csrc/jsp_stamps.h build/jsp_engine.o build/jsp_walk.o build/jsp_multi.o $(HOST_OBJ) $(HDR)
	@mkdir -p build/diag tools/bin/diag
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) -DJSP_STAMPS -c -o build/diag/k.o jobset_amd/csrc/jsp_kernels.hip
	$(HIPCC) $(HIPFLAGS) -shared -o $@ build/diag/k.o build/jsp_engine.o build/jsp_walk.o build/jsp_multi.o $(HOST_OBJ) -ldl

# ASan + UBSan build of the host mirror (webhook / reconciler / planner / JSON)
# linked with the product engine objects, and of the C oracles; tests/
# test_sanitizers.py runs the host and oracle suites against them under a
# preloaded libasan. Host code only: GPU sanitizers are not used.
SANFLAGS = -O1 -g -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -fsanitize=address,undefined \
	-fno-omit-frame-pointer -fno-sanitize-recover=undefined
ASAN_OBJ = $(patsubst jobset_amd/csrc/host/%.cc,build/asan/host_%.o,$(HOST_SRC))
sanitize: build/asan/libjsplace.so
	$(MAKE) -s -C oracle sanitize
build/asan/host_%.o: jobset_amd/csrc/host/%.cc $(HOST_HDR) $(HDR)
	@mkdir -p build/asan
	$(CXX) $(SANFLAGS) -c -o $@ $<
build/asan/libjsplace.so: build/jsp_kernels.o build/jsp_engine.o build/jsp_walk.o build/jsp_multi.o $(ASAN_OBJ)
	$(CXX) -shared -fsanitize=address,undefined -o $@ $^ -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64

# ASan + UBSan stand-alone driver of the planner's assume ledger (planner.assume
# / sync / planner.forget through jsk_host.h, no engine bound): the host mirror
# compiled with the sanitizers into one program with its own main, linked with
# the product engine objects it never calls into. Runs on the CPU.
tools/bin/ledger_san: tools/ledger_san.cc $(HOST_SRC) $(HOST_HDR) $(HDR) build/jsp_kernels.o build/jsp_engine.o build/jsp_walk.o build/jsp_multi.o
	@mkdir -p tools/bin
	$(CXX) $(SANFLAGS) -o $@ tools/ledger_san.cc $(HOST_SRC) build/jsp_kernels.o build/jsp_engine.o build/jsp_walk.o \
		build/jsp_multi.o -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64 -ldl -lpthread

# ThreadSanitizer build of the host mirror (the engine objects as built):
# tests/test_concurrency.py runs its concurrent host-mirror callers against it
# with libtsan preloaded. Host code only.
TSANFLAGS = -O1 -g -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -fsanitize=thread -fno-omit-frame-pointer
TSAN_OBJ = $(patsubst jobset_amd/csrc/host/%.cc,build/tsan/host_%.o,$(HOST_SRC))
tsan: build/tsan/libjsplace.so
build/tsan/host_%.o: jobset_amd/csrc/host/%.cc $(HOST_HDR) $(HDR)
	@mkdir -p build/tsan
	$(CXX) $(TSANFLAGS) -c -o $@ $<
build/tsan/libjsplace.so: build/jsp_kernels.o build/jsp_engine.o build/jsp_walk.o build/jsp_multi.o $(TSAN_OBJ)
	$(CXX) -shared -fsanitize=thread -o $@ $^ -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64 -ldl

# Stand-alone GPU probes (dispatch_probe, stream_ceiling, layout_probe,
# mailbox_probe, valu_rate, block_probe, stop_anatomy): make tools/bin/<name>
PROBE_LIBS_mailbox_probe = -lhsa-runtime64
tools/bin/%: tools/%.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -o $@ $< $(PROBE_LIBS_$*)

# The host's line functions alone (jsp_lines.h: the answer's expansion, the
# kept list's tag check and copy), stand-alone CPU programs: lines_bench times
# them on cfg2's line shape; lines-asan builds lines_check (the CPU cases of
# tests/test_lines_memo.py, output buffers of exactly J ints) with ASan + UBSan
# and runs it. CPU only.
tools/bin/lines_bench: tools/lines_bench.cc jobset_amd/csrc/jsp_lines.h
	@mkdir -p tools/bin
	$(HIPCC) -O3 -std=c++17 -o $@ $<
tools/bin/lines_check: tools/lines_check.cc jobset_amd/csrc/jsp_lines.h
	@mkdir -p tools/bin
	$(CXX) $(SANFLAGS) -o $@ $<
lines-asan: tools/bin/lines_check
	tools/bin/lines_check

# The waits' one loop alone (jsp_wait.h: guarded_wait and its pacer) with a
# scripted stream query and a clock the cases advance: every result and the
# beat, built with ASan + UBSan and run. CPU only, nothing sleeps.
tools/bin/wait_check: tools/wait_check.cc jobset_amd/csrc/jsp_wait.h
	@mkdir -p tools/bin
	$(CXX) $(SANFLAGS) -o $@ $<
wait-asan: tools/bin/wait_check
	tools/bin/wait_check

# The entry stamps' clock and the leased answers' metrics alone (jsp_clock.h,
# jsp_leased_metrics.h) under threads: clock_check built with ASan + UBSan and
# with TSan, each run directly. select_bench times the timing loops' median /
# p99 selection (jsp_select.h) against the sort it replaces. CPU only.
CLOCK_HDR = jobset_amd/csrc/jsp_clock.h jobset_amd/csrc/jsp_leased_metrics.h include/jsplace.h
tools/bin/clock_check_asan: tools/clock_check.cc $(CLOCK_HDR)
	@mkdir -p tools/bin
	$(CXX) $(SANFLAGS) -o $@ $< -lpthread
tools/bin/clock_check_tsan: tools/clock_check.cc $(CLOCK_HDR)
	@mkdir -p tools/bin
	$(CXX) $(TSANFLAGS) -o $@ $< -lpthread
clock-asan: tools/bin/clock_check_asan
	tools/bin/clock_check_asan
clock-tsan: tools/bin/clock_check_tsan
	tools/bin/clock_check_tsan
tools/bin/select_bench: tools/select_bench.cc jobset_amd/csrc/jsp_select.h
	@mkdir -p tools/bin
	$(CXX) -O2 -std=c++17 -o $@ $<

clean:
	rm -rf build $(LIB)
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean diag sanitize tsan lines-asan wait-asan clock-asan clock-tsan
