# libsamplers_hip.so — MI355X (gfx950) hot path.  `make` builds in-tree so the
# .so travels to the GPU box with the repo snapshot.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CXXFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-result
SRC := samplers_amd/csrc/sp_dps.hip samplers_amd/csrc/sp_blur.hip samplers_amd/csrc/sp_sr.hip \
       samplers_amd/csrc/sp_psf.hip samplers_amd/csrc/sp_phase.hip \
       samplers_amd/csrc/sp_psf_fft.hip samplers_amd/csrc/sp_radon.hip \
       samplers_amd/csrc/sp_svd_sep.hip samplers_amd/csrc/sp_hadamard.hip \
       samplers_amd/csrc/sp_chanmix.hip \
       samplers_amd/csrc/sp_latent.hip samplers_amd/csrc/sp_cg.hip \
       samplers_amd/csrc/sp_groupnorm.hip samplers_amd/csrc/sp_conv.hip \
       samplers_amd/csrc/sp_wino.hip samplers_amd/csrc/sp_conv_thin.hip \
       samplers_amd/csrc/sp_conv_s2.hip samplers_amd/csrc/sp_upsample.hip \
       samplers_amd/csrc/sp_attention.hip samplers_amd/csrc/sp_attention6.hip \
       samplers_amd/csrc/sp_gemm_x6.hip samplers_amd/csrc/sp_transformer.hip \
       samplers_amd/csrc/sp_bf16_conv.hip samplers_amd/csrc/sp_bf16_groupnorm.hip \
       samplers_amd/csrc/sp_bf16_rows.hip samplers_amd/csrc/sp_bf16_attention.hip
OBJ := $(patsubst samplers_amd/csrc/%.hip,build/%.o,$(SRC))
LIB := samplers_amd/lib/libsamplers_hip.so
# bounds-checked debug build (SP_DCHECK index / range invariants counted on the device,
# sp_debug_violations): same sources, -DSP_DEBUG=1, its own objects and library
DOBJ := $(patsubst samplers_amd/csrc/%.hip,build/debug/%.o,$(SRC))
DLIB := samplers_amd/lib/debug/libsamplers_hip.so

all: $(LIB) $(DLIB)

debug: $(DLIB)

# the Winograd tile's transforms stay scalar: packed f32 ops cost more than two scalar
# ones beside MFMAs (MI355X_MICROARCH price list)
build/sp_wino.o build/debug/sp_wino.o: EXTRA := -fno-slp-vectorize
# the PSF sweep's FMAs stay scalar too: packed, every odd tap needs its window pair re-aligned
# by moves (measured no faster at R = 30, 9-12 % slower at R <= 15)
build/sp_psf.o build/debug/sp_psf.o: EXTRA := -fno-slp-vectorize
# the attention kernels keep their accumulators in VGPRs: in the AGPR form the compiler copied
# every score / output block between the two register files around each MFMA; the bf16 conv tile
# was tuned under the same form (sp_bf16_groupnorm and sp_bf16_rows have no MFMA: their device
# code is the same either way)
VGPR_FORM := sp_attention sp_attention6 sp_bf16_conv sp_bf16_attention
$(VGPR_FORM:%=build/%.o) $(VGPR_FORM:%=build/debug/%.o): EXTRA := -mllvm -amdgpu-mfma-vgpr-form=1

build/%.o: samplers_amd/csrc/%.hip samplers_amd/csrc/sp_common.h samplers_amd/csrc/sp_ops.h samplers_amd/csrc/sp_fft.h samplers_amd/csrc/sp_bf16.h include/samplers_hip.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) $(EXTRA) -c $< -o $@

$(LIB): $(OBJ)
	@mkdir -p samplers_amd/lib
	$(HIPCC) -shared --offload-arch=$(ARCH) -o $@ $(OBJ)

build/debug/%.o: samplers_amd/csrc/%.hip samplers_amd/csrc/sp_common.h samplers_amd/csrc/sp_ops.h samplers_amd/csrc/sp_fft.h samplers_amd/csrc/sp_bf16.h include/samplers_hip.h
	@mkdir -p build/debug
	$(HIPCC) $(CXXFLAGS) $(EXTRA) -DSP_DEBUG=1 -c $< -o $@

$(DLIB): $(DOBJ)
	@mkdir -p samplers_amd/lib/debug
	$(HIPCC) -shared --offload-arch=$(ARCH) -o $@ $(DOBJ)

clean:
	rm -rf build $(LIB) $(DLIB)

.PHONY: all debug clean
