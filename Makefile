# Build libpromonet_hip.so (gfx950) and nothing else. `make -j4`.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
# TUNING=1: A/B scaffolding (PM_FUSION / PM_NO_NARROW / PM_FARGAN environment
# switches, phase-timeline stamps, ablation defines). Never in the shipped .so.
TUNING ?= 0
# A/B variants (scripts/build_variant.sh): more flags for every object, and
# OBJ / LIB on the command line for a build beside the shipped one
EXTRA ?=
CXXFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -Wno-unused-value -fno-honor-nans $(EXTRA)
ifeq ($(TUNING),1)
CXXFLAGS += -DPM_TUNING
endif
SRC = promonet_amd/csrc
OBJ = build/obj
LIB = promonet_amd/lib/libpromonet_hip.so
# every .hip is an object of the library: the one place that lists them
OBJS = $(patsubst $(SRC)/%.hip,$(OBJ)/%.o,$(sort $(wildcard $(SRC)/*.hip)))
# the spectral head keeps torch.clip's NaN (a NaN magnitude stays NaN)
$(OBJ)/pm_vocos.o: CXXFLAGS += -fhonor-nans
# the harmonic contours carry NaN (an unvoiced prior, a harmonic that is absent)
$(OBJ)/pm_harmonics.o: CXXFLAGS += -fhonor-nans
# NaN audio gives NaN LPC features; the lattice steps contract to fma. No SLP
# vectorisation: packed fp32 pairs break on the one-element shift of every
# order and cost 82 moves an order to re-pair (pm_lpc.h)
$(OBJ)/pm_lpc.o: CXXFLAGS += -fhonor-nans -fno-slp-vectorize
# the limiter is bit for bit the reference's: every product and sum rounds on
# its own (pm_limit.h)
$(OBJ)/pm_limit.o: CXXFLAGS += -ffp-contract=off
# the multi-tensor mean rounds every product and sum on its own, as the fp32
# restatement of its tests does; its division stays correctly rounded
# (pm_adv.h); the hinge of a NaN logit is NaN, as torch.clamp's is
$(OBJ)/pm_adv.o: CXXFLAGS += -ffp-contract=off -fhonor-nans
# torch's semantics on inf and NaN (pm_nonfinite.h): the
# ReLU of the FARGAN discriminator's layers, the decibel spectrogram's clamp,
# maximum and floor, and the spectral-convergence loss's clamp keep a NaN, so
# an overflow reaches the optimizer's scaler; without -fhonor-nans the tests
# of a NaN fold to false
$(OBJ)/pm_fdisc.o $(OBJ)/pm_disc_spec.o $(OBJ)/pm_loss.o: CXXFLAGS += -fhonor-nans
# the optimizer step is bit for bit its restatement (tests/optim_oracle.py):
# every fp32 and double product and sum rounds on its own, and a NaN gradient
# is counted: without -fhonor-nans the compiler reads the test of the exponent
# bits as |g| != inf and lets NaN pass (pm_optim.h)
$(OBJ)/pm_optim.o: CXXFLAGS += -ffp-contract=off -fhonor-nans
# the whole-MRF kernels: see pm_conv_bf16_mrf.hip
MRF_FLAGS ?= -mllvm -amdgpu-sched-strategy=max-ilp
HDRS = $(wildcard $(SRC)/*.h) include/promonet_hip.h

all: $(LIB)

$(OBJ)/%_mrf.o: $(SRC)/%_mrf.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(CXXFLAGS) $(MRF_FLAGS) -c $< -o $@

$(OBJ)/%.o: $(SRC)/%.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p $(dir $@)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -o $@
	@python3 scripts/check_spills.py $(OBJS) || true

# fails when any kernel spills VGPRs or uses scratch memory
check: $(LIB)
	python3 scripts/check_spills.py $(OBJS)

# the object list, for the scripts that link a variant of one object
objs:
	@echo $(OBJS)

clean:
	rm -rf build $(LIB)

# Micro-benchmarks behind DESIGN.md section 6 (run the binaries on the GPU box)
MICRO = mfma_peak mfma_shapes mma_loop phase_overlap overlap2 lds_dma xcd_exchange
micro: $(addprefix promonet_amd/lib/,$(MICRO))
promonet_amd/lib/%: scripts/micro/%.hip promonet_amd/csrc/pm_conv.h
	$(HIPCC) $(CXXFLAGS) -Wno-unused-result $< -o $@
