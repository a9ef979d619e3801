# Builds the REFERENCE's own test / validation / example programs, from their sources where they lie under
# $(REF), against OUR library (pffft_amd/libpffft_hip.so) instead of the reference's PFFFT/PFFASTCONV
# libraries: the drop-in claim of SURVEY.md row f-1.  Nothing of the reference is copied; only the
# executables land in oracle/_ref/bin/ (git-ignored; built next to the reference objects, they travel with them
# to the GPU box).  Run from oracle/:  make -C oracle -f refprogs.mk REF=<reference tree>
# The reference's headers (include/pffft/*.h, pffft.hpp) are used verbatim — they ARE the interface.
REF ?= /root/reference
ROOT := $(abspath ..)
OUT := $(ROOT)/oracle/_ref/bin
LIBDIR := $(ROOT)/pffft_amd
INC := -I$(REF)/include -I$(REF)/include/pffft -I$(REF)/src
LINK := -L$(LIBDIR) -lpffft_hip -Wl,-rpath,'$$ORIGIN/../../../pffft_amd' -Wl,-rpath,/opt/rocm/lib -lm
CFLAGS := -std=c99 -O2 -D_USE_MATH_DEFINES $(INC)
CXXFLAGS := -O2 -D_USE_MATH_DEFINES $(INC)

BINS := test_pffft_float test_pffft_double test_fft_factors test_pffastconv \
        bench_pffft_float bench_pffft_double test_pffft_cpp test_pffft_cpp11 \
        example_c_real_flt_fwd example_c_cplx_dbl_fwd example_cpp98_real_flt_fwd example_cpp11_cplx_dbl_fwd \
        example_cpp98_cplx_flt_fwd example_cpp11_real_dbl_fwd \
        bench_mixers

all: $(addprefix $(OUT)/,$(BINS))

$(OUT):
	mkdir -p $(OUT)

$(OUT)/test_pffft_float: $(REF)/tests/test_pffft.c | $(OUT)
	gcc $(CFLAGS) -DPFFFT_ENABLE_FLOAT -o $@ $< $(LINK)
$(OUT)/test_pffft_double: $(REF)/tests/test_pffft.c | $(OUT)
	gcc $(CFLAGS) -DPFFFT_ENABLE_DOUBLE -o $@ $< $(LINK)
$(OUT)/test_fft_factors: $(REF)/tests/test_fft_factors.c | $(OUT)
	gcc $(CFLAGS) -DPFFFT_ENABLE_FLOAT -DPFFFT_ENABLE_DOUBLE -o $@ $< $(LINK)
$(OUT)/test_pffastconv: $(REF)/tests/test_pffastconv.c | $(OUT)
	gcc $(CFLAGS) -o $@ $< $(LINK)
# bench_pffft --validate cross-checks against FFTPACK (the reference's own known-answer oracle): fftpack.c is
# compiled in as a CPU comparator exactly as benchmarks/CMakeLists.txt does
$(OUT)/bench_pffft_float: $(REF)/benchmarks/bench_pffft.c $(REF)/src/fftpack.c | $(OUT)
	gcc $(CFLAGS) -DPFFFT_ENABLE_FLOAT -DHAVE_FFTPACK=1 -o $@ $^ $(LINK)
$(OUT)/bench_pffft_double: $(REF)/benchmarks/bench_pffft.c $(REF)/src/fftpack.c | $(OUT)
	gcc $(CFLAGS) -DPFFFT_ENABLE_DOUBLE -DFFTPACK_DOUBLE_PRECISION -DHAVE_FFTPACK=1 -o $@ $^ $(LINK)
$(OUT)/test_pffft_cpp: $(REF)/tests/test_pffft.cpp | $(OUT)
	g++ -std=c++98 $(CXXFLAGS) -DPFFFT_ENABLE_FLOAT -DPFFFT_ENABLE_DOUBLE -o $@ $< $(LINK)
$(OUT)/test_pffft_cpp11: $(REF)/tests/test_pffft.cpp | $(OUT)
	g++ -std=c++11 $(CXXFLAGS) -DPFFFT_ENABLE_FLOAT -DPFFFT_ENABLE_DOUBLE -o $@ $< $(LINK)
$(OUT)/example_c_%: $(REF)/examples/example_c_%.c | $(OUT)
	gcc $(CFLAGS) -DPFFFT_ENABLE_FLOAT -DPFFFT_ENABLE_DOUBLE -o $@ $< $(LINK)
$(OUT)/example_cpp98_%: $(REF)/examples/example_cpp98_%.cpp | $(OUT)
	g++ -std=c++98 $(CXXFLAGS) -DPFFFT_ENABLE_FLOAT -DPFFFT_ENABLE_DOUBLE -o $@ $< $(LINK)
$(OUT)/example_cpp11_%: $(REF)/examples/example_cpp11_%.cpp | $(OUT)
	g++ -std=c++11 $(CXXFLAGS) -DPFFFT_ENABLE_FLOAT -DPFFFT_ENABLE_DOUBLE -o $@ $< $(LINK)

# the reference's only program over the PFDSP mixers (row f-4), against libpfdsp_hip.so instead of libpfdsp
$(OUT)/bench_mixers: $(REF)/benchmarks/bench_mixers.cpp | $(OUT)
	g++ -std=c++11 $(CXXFLAGS) -I$(REF)/benchmarks -o $@ $< -L$(LIBDIR) -lpfdsp_hip -Wl,-rpath,'$$ORIGIN/../../../pffft_amd' -Wl,-rpath,/opt/rocm/lib -lm

clean:
	rm -rf $(OUT)
.PHONY: all clean
