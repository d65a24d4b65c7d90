# test_host_align_wide (tests/test_host_cpp_wide_gpu.py): SparseImgAlignHip on a bundle with an equidistant or atan camera.
# A makefile of its own beside tests/cpp/Makefile, with that file's flags:  make -C tests/cpp -f align_wide.mk
ROOT := ../..
LIBS := -L$(ROOT)/svo_pro_universal_amd/host -lsvo_hip_host -L$(ROOT)/svo_pro_universal_amd/csrc -lsvo_hip \
  -Wl,-rpath,'$$ORIGIN/../../svo_pro_universal_amd/host' -Wl,-rpath,'$$ORIGIN/../../svo_pro_universal_amd/csrc'
DEPS := $(ROOT)/svo_pro_universal_amd/host/libsvo_hip_host.so $(ROOT)/svo_pro_universal_amd/csrc/libsvo_hip.so
all: test_host_align_wide
test_host_align_wide: test_host_align_wide.cpp $(DEPS)
	g++ -std=c++17 -O1 -Wall -o $@ $< $(LIBS)
clean:
	rm -f test_host_align_wide
.PHONY: all clean
