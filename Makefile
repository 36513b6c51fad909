# Build recipe for every native artefact (no cmake/ninja needed).
#   libfdf.so        HIP kernels + C ABI (the product), gfx950 only
#   liboracle.so     scalar C restatement of the reference semantics (test infrastructure)
#   libfast_avx2.so  C++ AVX2 port of the reference's fast_simd path (CPU baseline only)
#   tests/cpp/test_cpp_*   smoke binaries of the C++ API (include/fdf.hpp): detection,
#                          fdf::select_best, fdf::keypoint_angles, fdf::keypoint_harris,
#                          fdf::keypoint_descriptors,
#                          fdf::match_descriptors, fdf::resize / fdf::build_pyramid,
#                          fdf::estimate_model, fdf::refine_model, fdf::estimate_fundamental,
#                          fdf::warp,
#                          fdf::track, fdf::update_tracks
#   tests/cpp/test_wg_share  host-only check of the kernels' work split (fdf_common.h)
#   tests/cpp/test_geometry  host-only table of the band geometry and launch plan (fdf_geometry.h)
HIPCC ?= /opt/rocm/bin/hipcc
CC ?= gcc
CXX ?= g++
ARCH ?= gfx950

PKG := feature_detector_fast_amd
CSRC := $(PKG)/csrc
LIBFDF := $(PKG)/libfdf.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Iinclude $(EXTRA_HIPFLAGS)
OBJS := $(addprefix $(CSRC)/fdf_,$(addsuffix .o,kernels sweep sweep_latency sweep_rgb select \
	orient harris describe match ransac fundamental resize warp track tracks api stages pipeline))
HEADERS := $(wildcard $(CSRC)/*.h) include/fdf.h
CPP_TESTS := $(addprefix tests/cpp/test_cpp_,api select orient harris describe match pyramid ransac refine fundamental warp track tracks)

all: $(LIBFDF) oracle/liboracle.so oracle/libfast_avx2.so $(CPP_TESTS) tests/cpp/test_wg_share \
	tests/cpp/test_geometry

$(CSRC)/%.o: $(CSRC)/%.hip $(HEADERS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/%.o: $(CSRC)/%.cpp $(HEADERS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBFDF): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

oracle/liboracle.so: oracle/fast_oracle.c oracle/fast_oracle.h
	$(CC) -O2 -std=c11 -fPIC -shared -Wall -o $@ $<

oracle/libfast_avx2.so: oracle/fast_avx2.cpp
	$(CXX) -O3 -mavx2 -std=c++17 -fPIC -shared -Wall -o $@ $< -lpthread

tests/cpp/%: tests/cpp/%.cpp include/fdf.hpp include/fdf.h $(LIBFDF)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -o $@ $< -L$(PKG) -lfdf -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

# fdf_common.h is a HIP header: the compiler's host pass alone, no device code, no libfdf.so
tests/cpp/test_wg_share: tests/cpp/test_wg_share.cpp $(CSRC)/fdf_common.h $(CSRC)/fdf_kernels.h
	$(HIPCC) -x hip --offload-host-only -O2 -std=c++17 -Wall -o $@ $<

tests/cpp/test_geometry: tests/cpp/test_geometry.cpp $(CSRC)/fdf_geometry.h $(CSRC)/fdf_kernels.h include/fdf.h
	$(HIPCC) -x hip --offload-host-only -O2 -std=c++17 -Wall -o $@ $<

# Ablation build (tools/ablate.py, tools/pmc_ablate.sh): the same library with the internal
# FDF_DEBUG_FLAGS / FDF_NSUB / FDF_LDS_BUDGET / FDF_COMPACT_TPG switches compiled in.
debug: build/libfdf_debug.so

build/libfdf_debug.so: $(CSRC)/*.hip $(CSRC)/*.cpp $(CSRC)/*.h include/fdf.h
	bash tools/build_variant.sh debug "-DFDF_DEBUG_BUILD"

clean:
	rm -f $(CSRC)/*.o $(LIBFDF) oracle/*.so $(CPP_TESTS) tests/cpp/test_wg_share \
		tests/cpp/test_geometry

.PHONY: all clean debug
