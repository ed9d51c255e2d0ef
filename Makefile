# Builds everything in-tree (the .so files travel to the GPU box with the snapshot).
#   libtrt_hip.so   — the C-ABI hot path (include/trt.h), HIP for gfx950
#   libtrt_lbvh.so  — GPU BVH builder (include/trt_build.h), HIP for gfx950; not needed by the render path
#   libtrt_host.so  — loaders / BVH / PNG (include/trt_host.h), plain C++
#   tinyrt          — CLI: loaders -> render() -> PNG (the reference's main())
#   oracle/liboracle.so — CPU restatement used by tests/ and bench.py only
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
PKG := tinyraytracing_amd
OUT := $(PKG)/lib

# Bit-parity rule (include/trt_prims.h): no FP contraction on either side;
# FMA only where the source says fmaf.  x86-64-v3 = AVX2 + hardware FMA.
CPU_FP := -ffp-contract=off -march=x86-64-v3
CXXFLAGS := -O2 -g0 -std=c++17 -fPIC -Wall -Wextra $(CPU_FP) -Iinclude -I$(PKG)/host
# The LLVM atomic optimizer turns the one-lane queue reservation of k_shade (blockStage) into "atomic; s_waitcnt vmcnt(0);
# readfirstlane", i.e. waits for the round trip (and every store before it) on the spot; the kernel consumes the value one
# stage later.  No kernel here relies on that pass: every atomic is issued by one lane per wave already.
# -fno-slp-vectorize: left to itself the SLP vectoriser pairs the scalar fp32 operations of the triangle test and of the shading
# code into v_pk_* instructions; on gfx950 a v_pk_mul/add costs what two v_mul/add cost (tools/valu_probe.hip: 4.6 against
# 2 x 2.4 clocks per wave) and the pairs have to be assembled with v_mov first: trace_closest on `back` -9 %, k_shade -3 %.
# (The explicit two-wide code of innerStep() is not affected: its operands are loaded as pairs.)
HIPFLAGS := -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize \
            -mllvm -amdgpu-atomic-optimizer-strategy=None \
            -Wall -Wextra -Wno-unused-parameter -Iinclude -I$(PKG)/csrc

HOST_SRC := $(PKG)/host/scene.cpp $(PKG)/host/bvh.cpp $(PKG)/host/synth.cpp $(PKG)/host/image_out.cpp $(PKG)/host/jpeg.cpp $(PKG)/host/png.cpp $(PKG)/host/capi.cpp
HOST_HDR := $(wildcard $(PKG)/host/*.h) $(wildcard $(PKG)/csrc/*.h) include/trt.h include/trt_host.h include/trt_prims.h include/trt_exact.h
HIP_SRC := $(PKG)/csrc/trt_api.hip
HIP_HDR := $(wildcard $(PKG)/csrc/*.h) include/trt.h include/trt_prims.h include/trt_exact.h

# test-only library of tests/test_shade_cases_cpu.py: part of `all` wherever its source is in the tree
SHADE_MUTANTS := $(if $(wildcard tests/hostsim/shade_mutants.cpp),shademutants)

.PHONY: all host hip lbvh oracle cli hostsim denoisecpu reprojectcpu motioncpu momentscpu despecklecpu refitcpu rayscpu cullcpu schedcpu onelightcpu nearlightscpu variants probe exactcheck nodecheck shadecheck shademutants clean
all: host hip lbvh oracle hostsim denoisecpu reprojectcpu motioncpu momentscpu despecklecpu refitcpu rayscpu cullcpu schedcpu onelightcpu nearlightscpu cli exactcheck nodecheck shadecheck $(SHADE_MUTANTS)

host: $(OUT)/libtrt_host.so
hip: $(OUT)/libtrt_hip.so
lbvh: $(OUT)/libtrt_lbvh.so
cli: $(OUT)/tinyrt
oracle:
	$(MAKE) -C oracle
# CPU compile of the device-side path functions, for tests only (tests/hostsim)
hostsim: tests/hostsim/libhostsim.so
tests/hostsim/libhostsim.so: tests/hostsim/hostsim.cpp $(wildcard tests/hostsim/*.h) $(wildcard tests/refit/*.h) tools/shade_cases.h $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/hostsim/hostsim.cpp
# deliberately altered copies of shading and light-picking functions run through the sections of tools/shade_cases.h, for the sensitivity check of tests/test_shade_cases_cpu.py
shademutants: tests/hostsim/libshade_mutants.so
tests/hostsim/libshade_mutants.so: tests/hostsim/shade_mutants.cpp tests/hostsim/shade_cases_host.h tools/shade_cases.h $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/hostsim/shade_mutants.cpp
# CPU compile of the a-trous filter's per-pixel code (trt_denoise.h), for tests only (tests/test_*denoise*.py)
denoisecpu: tests/denoise/libdenoise_cpu.so
tests/denoise/libdenoise_cpu.so: tests/denoise/denoise_cpu.cpp $(PKG)/csrc/trt_denoise.h include/trt.h include/trt_prims.h include/trt_exact.h
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/denoise/denoise_cpu.cpp
# CPU compile of trt_reproject's per-pixel code (trt_reproject.h), for tests only (tests/test_*reproject*.py)
reprojectcpu: tests/reproject/libreproject_cpu.so
tests/reproject/libreproject_cpu.so: tests/reproject/reproject_cpu.cpp $(PKG)/csrc/trt_reproject.h $(PKG)/csrc/trt_denoise.h include/trt.h include/trt_prims.h include/trt_exact.h
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/reproject/reproject_cpu.cpp
# CPU compile of trt_reproject_motion's per-pixel code (trt_reproject.h) and of trt_trace_points' hitPoint (trt_path.h), for tests only (tests/test_*motion*.py)
motioncpu: tests/motion/libmotion_cpu.so
tests/motion/libmotion_cpu.so: tests/motion/motion_cpu.cpp $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/motion/motion_cpu.cpp
# CPU compile of trt_reproject_moments' per-pixel code (trt_moments.h), for tests only (tests/test_*moments*.py)
momentscpu: tests/moments/libmoments_cpu.so
tests/moments/libmoments_cpu.so: tests/moments/moments_cpu.cpp $(PKG)/csrc/trt_moments.h $(PKG)/csrc/trt_reproject.h $(PKG)/csrc/trt_denoise.h include/trt.h include/trt_prims.h include/trt_exact.h
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/moments/moments_cpu.cpp
# CPU compile of trt_despeckle's per-pixel code (trt_despeckle.h), for tests only (tests/test_*despeckle*.py)
despecklecpu: tests/despeckle/libdespeckle_cpu.so
tests/despeckle/libdespeckle_cpu.so: tests/despeckle/despeckle_cpu.cpp $(PKG)/csrc/trt_despeckle.h $(PKG)/csrc/trt_denoise.h include/trt.h include/trt_prims.h include/trt_exact.h
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/despeckle/despeckle_cpu.cpp
# CPU compile of the geometry update's per-node functions (trt_refit.h) over collapseBvh / buildOct output, for tests only (tests/test_refit_cpu.py)
refitcpu: tests/refit/librefit_cpu.so
tests/refit/librefit_cpu.so: tests/refit/refit_cpu.cpp $(wildcard tests/refit/*.h) $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -pthread -I$(PKG)/csrc -shared -o $@ tests/refit/refit_cpu.cpp
# CPU compile of the per-ray functions of trt_render_rays (trt_path.h: rayRecord, rayValid, cameraRecord), for tests only (tests/test_render_rays_cpu.py)
rayscpu: tests/render_rays/librays_cpu.so
tests/render_rays/librays_cpu.so: tests/render_rays/rays_cpu.cpp $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -I$(PKG)/csrc -shared -o $@ tests/render_rays/rays_cpu.cpp
# CPU compile of the camera-ray cull bound (trt_cull.h) beside cameraRay and the two slab tests (trt_path.h), for tests only (tests/test_cull_cpu.py)
cullcpu: tests/cull/libcull_cpu.so
tests/cull/libcull_cpu.so: tests/cull/cull_cpu.cpp $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -I$(PKG)/csrc -shared -o $@ tests/cull/cull_cpu.cpp
# CPU compile of the shadow-queue placement of the render loop (trt_sched.h), for tests only (tests/test_sched_cpu.py)
schedcpu: tests/sched/libsched_cpu.so
tests/sched/libsched_cpu.so: tests/sched/sched_cpu.cpp $(PKG)/csrc/trt_sched.h
	$(CXX) $(CXXFLAGS) -I$(PKG)/csrc -shared -o $@ tests/sched/sched_cpu.cpp
# CPU build of TRT_FLAG_ONE_LIGHT: hostsim_render's loop with the light loop replaced by lightPick -> lightSample -> occlusion test, for tests only (tests/test_*one_light*.py)
onelightcpu: tests/onelight/libonelight_cpu.so
tests/onelight/libonelight_cpu.so: tests/onelight/onelight_cpu.cpp tests/hostsim/hostsim.cpp $(wildcard tests/hostsim/*.h) $(wildcard tests/refit/*.h) tools/shade_cases.h $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/onelight/onelight_cpu.cpp
# CPU build of TRT_FLAG_NEAR_LIGHTS: the same loop with the light picked by lightPickNear on buildLightTree's tree, for tests only (tests/test_*near_lights*.py)
nearlightscpu: tests/nearlights/libnearlights_cpu.so
tests/nearlights/libnearlights_cpu.so: tests/nearlights/nearlights_cpu.cpp tests/hostsim/hostsim.cpp $(wildcard tests/hostsim/*.h) $(wildcard tests/refit/*.h) tools/shade_cases.h $(HIP_HDR)
	$(CXX) $(CXXFLAGS) -fopenmp -I$(PKG)/csrc -shared -o $@ tests/nearlights/nearlights_cpu.cpp

$(OUT)/libtrt_host.so: $(HOST_SRC) $(HOST_HDR)
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) -I$(PKG)/csrc -fopenmp -shared -o $@ $(HOST_SRC)

$(OUT)/libtrt_hip.so: $(HIP_SRC) $(HIP_HDR)
	@mkdir -p $(OUT)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(HIP_SRC)

# -ffp-contract=off like every other library here: contraction would only move Morton codes and SAH costs, i.e. topology, but the tree is part of
# the checkpoint's scene hash and should not depend on the compiler's choice of fused operations.
$(OUT)/libtrt_lbvh.so: $(PKG)/csrc/trt_lbvh.hip include/trt.h include/trt_build.h
	@mkdir -p $(OUT)
	$(HIPCC) -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wall -Wextra -Wno-unused-parameter -Iinclude -shared -o $@ $(PKG)/csrc/trt_lbvh.hip

# tinyrt does not link libtrt_lbvh.so: render() dlopens it when --gpu-bvh asks for the device builder (include/trt_build.h)
$(OUT)/tinyrt: $(PKG)/host/main.cpp $(PKG)/host/render.cpp $(HOST_HDR) include/trt_build.h $(OUT)/libtrt_host.so $(OUT)/libtrt_hip.so
	$(CXX) $(CXXFLAGS) -o $@ $(PKG)/host/main.cpp $(PKG)/host/render.cpp -L$(OUT) -ltrt_host -ltrt_hip -fopenmp -ldl -Wl,-rpath,'$$ORIGIN'

# A/B builds of the HIP library for tuning on the GPU box: TRT_HIP_LIB=<path> selects one at run time.
# name=defines, "+" separating the -D options
# (round 4's k_shade occupancy arms — block sizes 256 / 512 / 640 / 768 at 4, 5 and 6 waves per SIMD — are on record in profiles/r04_ab_shade_tail.txt; what
# won is in the default build: TRT_SHADE1_* / TRT_SHADEN_* in trt_kernels.h.  shade_old = round 3's configuration for the A/B.)
VARIANTS := w8=-DTRT_TRACE_MINWAVES=8 nt0=-DTRT_NT=0 nt15=-DTRT_NT=15 shade_old=-DTRT_SHADE1_BLOCK=512+-DTRT_SHADE1_WAVES=4+-DTRT_SHADEN_BLOCK=512+-DTRT_SHADEN_WAVES=4 shadep256=-DTRT_SHADEP_BLOCK=256+-DTRT_SHADEP_WAVES=5
variants: $(HIP_SRC) $(HIP_HDR)
	@mkdir -p $(OUT)/variants
	@for v in $(VARIANTS); do name=$${v%%=*}; defs=$$(echo "$${v#*=}" | tr '+' ' '); \
	  echo "variant $$name: $$defs"; $(HIPCC) $(HIPFLAGS) $$defs -shared -o $(OUT)/variants/libtrt_hip_$$name.so $(HIP_SRC) || exit 1; done

clean:
	rm -rf $(OUT) tests/hostsim/libhostsim.so tests/hostsim/libshade_mutants.so tests/denoise/libdenoise_cpu.so tests/reproject/libreproject_cpu.so tests/motion/libmotion_cpu.so tests/moments/libmoments_cpu.so tests/despeckle/libdespeckle_cpu.so tests/refit/librefit_cpu.so tests/render_rays/librays_cpu.so tests/cull/libcull_cpu.so tests/sched/libsched_cpu.so tests/onelight/libonelight_cpu.so tests/nearlights/libnearlights_cpu.so
	$(MAKE) -C oracle clean

# exhaustive (2^32 inputs) proof that include/trt_exact.h returns the bits of sqrtf / 1.0f / sqrtf: run by tests/test_gpu_parity.py
exactcheck: tools/exact_unary_check
tools/exact_unary_check: tools/exact_unary_check.hip include/trt_exact.h include/trt_prims.h
	$(HIPCC) -O3 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Iinclude -o $@ tools/exact_unary_check.hip

# octVisit, innerStep and the box tests as gfx950 compiles them (the flags of the library), one thread per case: run by tests/test_gpu_node_claims.py
nodecheck: tools/node_visit_check
tools/node_visit_check: tools/node_visit_check.hip $(HIP_HDR)
	$(HIPCC) $(HIPFLAGS) -o $@ tools/node_visit_check.hip

# the shading functions (cameraRay, makeVertex, lightSample, nextRay, sampleDir, shadeBegin / shadeNext), the light pickers (lightPickAt, lightNodeStep, lightPickNear) and the primitives under them as gfx950 compiles
# them (the flags of the library), one thread per case, and digests over all 2^24 uniforms: run by tests/test_gpu_shade_cases.py
shadecheck: tools/shade_case_check
tools/shade_case_check: tools/shade_case_check.hip tools/shade_cases.h $(HIP_HDR)
	$(HIPCC) $(HIPFLAGS) -o $@ tools/shade_case_check.hip

# chip-ceiling probe + TCC counter calibration workload (tools/calibrate_counters.sh runs it on the GPU box)
probe: tools/gather_probe
tools/gather_probe: tools/gather_probe.hip
	$(HIPCC) -O3 --offload-arch=gfx950 -o $@ tools/gather_probe.hip
