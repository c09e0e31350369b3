# Builds, in-tree:
#   simple-path-tracer_amd/lib/libspt_host.so  host side (scene JSON/OBJ/EXR -> spt_scene_desc, PNG)
#   simple-path-tracer_amd/lib/libspt_hip.so   HIP kernels + C ABI (gfx950)
#   simple-path-tracer_amd/lib/libspt_hip_bez.so  the same with the Bezier-patch primitive (opened by libspt_hip.so on demand)
#   simple-path-tracer_amd/lib/spt             CLI with the reference's flags (src/main.rs:26-41)
#   oracle/liboracle.so                        CPU oracle (test infrastructure only)
# FP contraction is disabled everywhere so the deterministic math of
# include/spt_detmath.h gives identical bits on x86-64 and gfx950.
PKG      := simple-path-tracer_amd
LIBDIR   := $(PKG)/lib
CXX      ?= g++
HIPCC    ?= hipcc
CXXFLAGS := -std=c++17 -O2 -fPIC -Wall -Wextra -ffp-contract=off -fno-fast-math -Iinclude
# -fno-slp-vectorize: the SLP vectoriser pairs scalar f32 operations into v_pk_mul_f32 / v_pk_add_f32.  On gfx950 a packed
# f32 instruction issues in 4 cycles per wave64 (profiles/r03_issue_rate.md) - no better than two 2-cycle VOP2s - and every
# pair costs v_mov / v_pk_mov shuffles to line its operands up.  MEASURED (round 3): cfg2 81.3 -> 88.8 Gsamples/s, cfg4
# 91.9 -> 88.2 ms, cfg5 143.3 -> 138.6 ms, same bits (packed and scalar IEEE operations round alike).
HIPFLAGS := -std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize \
            -Wall -Wno-unused-function -Iinclude

# (multi_film_selftest.cpp has a main of its own: `make selftest`)
SELFTEST_SRC := $(PKG)/csrc/host/multi_film_selftest.cpp
HOST_SRC := $(filter-out $(SELFTEST_SRC),$(wildcard $(PKG)/csrc/host/*.cpp))
HOST_HDR := $(wildcard $(PKG)/csrc/host/*.hpp) $(wildcard include/*.h)
HIP_SRC  := $(wildcard $(PKG)/csrc/hip/*.hip)
HIP_HDR  := $(wildcard $(PKG)/csrc/hip/*.h) $(wildcard include/*.h)

.PHONY: all host hip hip-plain cli oracle selftest out-layout-check scene-build-check scene-deform-refit-check mesh-assemble-check bake-check probe-check clean
all: host oracle hip cli

host: $(LIBDIR)/libspt_host.so
hip: $(LIBDIR)/libspt_hip.so $(LIBDIR)/libspt_hip_bez.so
hip-plain: $(LIBDIR)/libspt_hip.so   # kernel iteration: the library every scene without Bezier patches uses
cli: $(LIBDIR)/spt
oracle:
	$(MAKE) -C oracle

$(LIBDIR)/libspt_host.so: $(HOST_SRC) $(HOST_HDR)
	@mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRC) -lz -lpthread

# one object per translation unit (spt_hip.hip = the runtime side: device, streams, uploads, scheduling + film kernels,
# inst_*.hip = groups of kernel instantiations, see csrc/hip/kernel_list.h; scene_build.cpp = the scene builder, host code
# without a HIP call, see csrc/hip/scene_build.h), compiled side by side with `make -jN`
OBJDIR   := build/hip
BUILD_SRC := $(PKG)/csrc/hip/scene_build.cpp
BUILD_OBJ := $(OBJDIR)/scene_build.o
HIP_OBJ     := $(patsubst $(PKG)/csrc/hip/%.hip,$(OBJDIR)/plain/%.o,$(HIP_SRC)) $(BUILD_OBJ)
HIP_OBJ_BEZ := $(patsubst $(PKG)/csrc/hip/%.hip,$(OBJDIR)/bez/%.o,$(HIP_SRC)) $(BUILD_OBJ)

# the builder's float arithmetic (box padding, SAH costs, the 4-wide quantisation) reaches the films: the compiler, the mode and
# the flags of the host side of spt_hip.hip, and that side alone (no device pass).  Nothing in it depends on SPT_WITH_BEZIER, so both libraries link the one object
$(BUILD_OBJ): $(BUILD_SRC) $(HIP_HDR)
	@mkdir -p $(dir $@)
	$(HIPCC) -x hip --offload-host-only $(HIPFLAGS) -c -o $@ $<

$(OBJDIR)/plain/%.o: $(PKG)/csrc/hip/%.hip $(HIP_HDR)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# the same sources with the CubicBezier primitive compiled in; the library is opened by libspt_hip.so for scenes with patches
$(OBJDIR)/bez/%.o: $(PKG)/csrc/hip/%.hip $(HIP_HDR)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -DSPT_WITH_BEZIER=1 -c -o $@ $<

$(LIBDIR)/libspt_hip.so: $(HIP_OBJ)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -Wl,-Bsymbolic -o $@ $(HIP_OBJ) -ldl

$(LIBDIR)/libspt_hip_bez.so: $(HIP_OBJ_BEZ)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -Wl,-Bsymbolic -o $@ $(HIP_OBJ_BEZ) -ldl

$(LIBDIR)/spt: $(PKG)/csrc/cli/main.cpp $(wildcard include/*.h) $(LIBDIR)/libspt_host.so $(LIBDIR)/libspt_hip.so
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(LIBDIR) -lspt_host -lspt_hip -Wl,-rpath,'$$ORIGIN'

# The film fan-out of multi.cpp with stand-in devices, once under ThreadSanitizer and once under AddressSanitizer + UBSan: host code
# only, stand-alone programs with the sanitizer runtimes linked in (tests/test_multi_film_selftest.py runs them)
SELFTEST_DIR := build/selftest
selftest: $(SELFTEST_DIR)/multi_film_selftest_tsan $(SELFTEST_DIR)/multi_film_selftest_asan

$(SELFTEST_DIR)/multi_film_selftest_tsan: $(SELFTEST_SRC) $(PKG)/csrc/host/multi.cpp $(wildcard include/*.h)
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -Iinclude -fsanitize=thread -static-libtsan -o $@ $(SELFTEST_SRC) $(PKG)/csrc/host/multi.cpp -lpthread

$(SELFTEST_DIR)/multi_film_selftest_asan: $(SELFTEST_SRC) $(PKG)/csrc/host/multi.cpp $(wildcard include/*.h)
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -Iinclude -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ $(SELFTEST_SRC) $(PKG)/csrc/host/multi.cpp -lpthread

# csrc/hip/out_layout.h (where k_finish_host stores a film's floats) against a plain loop over rows, under AddressSanitizer + UBSan:
# a stand-alone host program (tests/test_out_layout.py runs it)
out-layout-check: $(SELFTEST_DIR)/out_layout_check
$(SELFTEST_DIR)/out_layout_check: tests/out_layout_check.cpp $(PKG)/csrc/hip/out_layout.h
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ $<

# The scene builder on its own, under AddressSanitizer + UBSan, over scene files that libspt_host.so loads: layout, references,
# "an update writes what a creation writes", determinism and the refusals (tests/test_scene_build.py writes the scenes and runs it)
ROCM_PATH ?= $(shell hipconfig --rocmpath 2>/dev/null || echo /opt/rocm)
scene-build-check: $(SELFTEST_DIR)/scene_build_check
$(SELFTEST_DIR)/scene_build_check: tests/scene_build_check.cpp $(BUILD_SRC) $(HIP_HDR) $(LIBDIR)/libspt_host.so
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math -Iinclude -I$(PKG)/csrc/hip -D__HIP_PLATFORM_AMD__ -isystem $(ROCM_PATH)/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ tests/scene_build_check.cpp $(BUILD_SRC) \
	    -L$(LIBDIR) -lspt_host -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# The refit arithmetic of spt_scene_deform's kernels (csrc/hip/scene_refit.h) under the kernels' level schedule, on the CPU, over
# trees the builder makes: a stand-alone host program under AddressSanitizer + UBSan (tests/test_scene_deform_refit.py runs it)
scene-deform-refit-check: $(SELFTEST_DIR)/scene_deform_refit_check
$(SELFTEST_DIR)/scene_deform_refit_check: tests/scene_deform_refit_check.cpp $(BUILD_SRC) $(HIP_HDR)
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math -Iinclude -I$(PKG)/csrc/hip -D__HIP_PLATFORM_AMD__ -isystem $(ROCM_PATH)/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ tests/scene_deform_refit_check.cpp $(BUILD_SRC)

# include/spt_mesh_assemble.h (the arithmetic of spt_scene_deform_vertices' kernels) against the loader's own calc_tangents and
# face_records (linked from libspt_host.so, as scene-build-check links it), by the kernels' schedule, over random meshes: a
# stand-alone host program under AddressSanitizer + UBSan (tests/test_mesh_assemble.py runs it)
mesh-assemble-check: $(SELFTEST_DIR)/mesh_assemble_check
$(SELFTEST_DIR)/mesh_assemble_check: tests/mesh_assemble_check.cpp $(HOST_HDR) $(LIBDIR)/libspt_host.so
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math -Iinclude \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ tests/mesh_assemble_check.cpp \
	    -L$(LIBDIR) -lspt_host -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# include/spt_bake.h on the host and the lightmap rasteriser (csrc/host/bake.cpp, compiled into the program itself; the loader comes
# from libspt_host.so, as mesh-assemble-check links it): a stand-alone host program under AddressSanitizer + UBSan
# (tests/test_bake_host.py runs it)
bake-check: $(SELFTEST_DIR)/bake_check
$(SELFTEST_DIR)/bake_check: tests/bake_check.cpp $(PKG)/csrc/host/bake.cpp $(HOST_HDR) $(LIBDIR)/libspt_host.so
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math -Iinclude \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ tests/bake_check.cpp $(PKG)/csrc/host/bake.cpp \
	    -L$(LIBDIR) -lspt_host -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# include/spt_probe.h on the host and the host entry points of csrc/host/probe.cpp (compiled into the program itself; the error
# channel comes from libspt_host.so) over degenerate inputs: a stand-alone host program under AddressSanitizer + UBSan
# (tests/test_probe_host.py runs it)
probe-check: $(SELFTEST_DIR)/probe_check
$(SELFTEST_DIR)/probe_check: tests/probe_check.cpp $(PKG)/csrc/host/probe.cpp $(HOST_HDR) $(LIBDIR)/libspt_host.so
	@mkdir -p $(SELFTEST_DIR)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fno-fast-math -Iinclude \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ tests/probe_check.cpp $(PKG)/csrc/host/probe.cpp \
	    -L$(LIBDIR) -lspt_host -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

clean:
	rm -rf $(LIBDIR) build oracle/*.so oracle/_ref
