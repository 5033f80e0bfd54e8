# Build libpgx.so (HIP for gfx950) and the C oracle twin.  `make -j8`
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -Wno-unused-variable
CSRC = pinot_amd/csrc
HDR = include/pgx.h $(CSRC)/pgx_internal.h $(CSRC)/pgx_jit_abi.h
HOST_HDR = $(HDR) $(CSRC)/pgx_host.h
# what every .hip file includes; SEL_HDR: the walk over the query kernels' selection bits
DEV_HDR = $(CSRC)/pgx_device.h $(CSRC)/pgx_internal.h $(CSRC)/pgx_jit_abi.h
SEL_HDR = $(DEV_HDR) $(CSRC)/pgx_hll_device.h

all: pinot_amd/libpgx.so

# The query compiler pastes these headers in front of every generated kernel: embed them as raw string literals.
build/%.inc: $(CSRC)/%.h
	@mkdir -p build
	@(echo 'R"PGXSRC('; cat $<; echo ')PGXSRC"') > $@

build/pgx_host.o: $(CSRC)/pgx_host.cpp $(HOST_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_part.o build/pgx_multi.o build/pgx_realtime.o build/pgx_fixtures.o build/pgx_stage.o build/pgx_mv.o build/pgx_select.o build/pgx_hll.o build/pgx_distinct.o build/pgx_percentile.o build/pgx_fasthll.o build/pgx_plan_cache.o build/pgx_plan.o: build/%.o: $(CSRC)/%.cpp $(HOST_HDR) $(CSRC)/pgx_hash.h $(CSRC)/pgx_sel_key.h
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_jit.o: $(CSRC)/pgx_jit.cpp $(HDR) build/pgx_jit_abi.inc build/pgx_device.inc build/pgx_roaring_device.inc build/pgx_jit_device.inc
	$(HIPCC) $(HIPFLAGS) -Ibuild -c $< -o $@

build/pgx_kernels.o: $(CSRC)/pgx_kernels.hip $(HDR) $(DEV_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_stats.o: $(CSRC)/pgx_stats.cpp $(CSRC)/pgx_internal.h
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_trim.o: $(CSRC)/pgx_trim.hip $(CSRC)/pgx_device.h
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_merge.o: $(CSRC)/pgx_merge.hip $(CSRC)/pgx_device.h
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_narrow.o: $(CSRC)/pgx_narrow.hip $(DEV_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_select_hip.o: $(CSRC)/pgx_select.hip $(DEV_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_hll_hip.o: $(CSRC)/pgx_hll.hip $(SEL_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_unpack_check.o: $(CSRC)/pgx_unpack_check.hip $(CSRC)/pgx_jit_device.h $(DEV_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_roaring.o: $(CSRC)/pgx_roaring.hip $(CSRC)/pgx_roaring_device.h $(DEV_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_distinct_hip.o: $(CSRC)/pgx_distinct.hip $(SEL_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_percentile_hip.o: $(CSRC)/pgx_percentile.hip $(SEL_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/pgx_fasthll_hip.o: $(CSRC)/pgx_fasthll.hip $(DEV_HDR)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

pinot_amd/libpgx.so: build/pgx_host.o build/pgx_part.o build/pgx_multi.o build/pgx_realtime.o build/pgx_fixtures.o build/pgx_stage.o build/pgx_mv.o build/pgx_plan_cache.o build/pgx_plan.o build/pgx_jit.o build/pgx_kernels.o build/pgx_trim.o build/pgx_stats.o build/pgx_merge.o build/pgx_narrow.o build/pgx_select_hip.o build/pgx_select.o build/pgx_hll_hip.o build/pgx_hll.o build/pgx_distinct_hip.o build/pgx_distinct.o build/pgx_percentile_hip.o build/pgx_percentile.o build/pgx_fasthll_hip.o build/pgx_fasthll.o build/pgx_roaring.o build/pgx_unpack_check.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ -L/opt/rocm/lib -lhiprtc -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined

# Host-only check of pgx_hash.h (the Java hash codes, the sort + unique union) under AddressSanitizer and UBSan: no device
# and of pgx_sel_key.h (the sparse GROUP BY's directory key); fasthll_host_check: the FASTHLL decode of pgx_hash.h
host-check: tests/host/distinct_host_check.cpp tests/host/sel_key_host_check.cpp tests/host/fasthll_host_check.cpp $(CSRC)/pgx_hash.h $(CSRC)/pgx_sel_key.h
	@mkdir -p build
	$(CXX) -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) tests/host/distinct_host_check.cpp -o build/distinct_host_check
	build/distinct_host_check
	$(CXX) -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) tests/host/sel_key_host_check.cpp -o build/sel_key_host_check
	build/sel_key_host_check
	$(CXX) -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) tests/host/fasthll_host_check.cpp -o build/fasthll_host_check
	build/fasthll_host_check

clean:
	rm -rf build pinot_amd/libpgx.so

.PHONY: all clean host-check
