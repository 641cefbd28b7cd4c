# Build of the MI355X-native Cassie physics library and its test infrastructure.
#
#   make            product library  cassie-mujoco-sim_amd/lib/libcassiemujoco.so   (hipcc, gfx950)
#   make oracle     CPU oracle       oracle/libcassie_oracle.so                     (gcc, test-only)
#   make emu        wave emulator    tests/emu/libcassie_emu.so                     (g++, test-only)
#                   + wave checks    tests/device/libwave_check.so                  (hipcc, gfx950, test-only)
#   make models     models/*.cmodel from the reference MJCF (needs /root/reference)
#
# The Agility blocks (pd_input / cassie_core_sim / state_output + pack/unpack) exist
# only as the closed static library shipped with the reference
# (src/libagilitycassie.a); it is whole-archived into the product .so exactly like
# the reference's own Makefile does (reference Makefile:18).  Where the reference tree
# is absent, the copy oracle/build_ref.sh staged in the git-ignored oracle/_ref/ is
# linked.  With neither, the product is linked with stand-ins for the archive's entry
# points that stop the process with a message when called (see AGILITY_ABSENT).

ROCM      ?= /opt/rocm
HIPCC     ?= $(ROCM)/bin/hipcc
ARCH      ?= gfx950
REF       ?= /root/reference
AGILITY   ?= $(REF)/src/libagilitycassie.a

PKG   := cassie-mujoco-sim_amd
CSRC  := $(PKG)/csrc
LIBD  := $(PKG)/lib
OBJD  := build

CXXFLAGS := -O2 -std=c++17 -fPIC -Iinclude -I$(CSRC)
CFLAGS   := -O2 -std=gnu11 -fPIC -Iinclude -I$(CSRC)
# -amdgpu-sched-strategy=iterative-ilp: the step kernel is one long latency-bound instruction stream at one wave per SIMD;
# scheduling for ILP instead of for occupancy measured +1.8 % (exact-pd) / +2.7 % (drive-pd), profiles/round2/README.md
# -disable-machine-licm: the substep loop is one 20 000-instruction body at the register limit; machine-level LICM hoists the
# materialisation of every fp64 literal and every loop-invariant lane predicate out of it -- into registers the loop does not
# have, i.e. into scratch and SGPR-spill lanes that the loop then reloads.  Without it: scratch 136 -> 0 B, 474 -> 392 SGPR
# spills, and +1 % (profiles/round3/README.md)
HIPFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Iinclude -I$(CSRC) -ffp-contract=on -mllvm -amdgpu-sched-strategy=iterative-ilp \
            -mllvm -disable-machine-licm

HOST_CPP := $(CSRC)/mjcf_loader.cpp $(CSRC)/phys_host.cpp
HOST_C   := $(wildcard $(CSRC)/*.c)
HIP_SRC  := $(wildcard $(CSRC)/*.hip)   # phys_batch.hip + one kernels_*.hip per model family (they compile side by side)
OBJS     := $(patsubst $(CSRC)/%.cpp,$(OBJD)/%.o,$(HOST_CPP)) $(patsubst $(CSRC)/%.c,$(OBJD)/%.o,$(HOST_C)) \
            $(patsubst $(CSRC)/%.hip,$(OBJD)/%.hip.o,$(HIP_SRC))

PRODUCT := $(LIBD)/libcassiemujoco.so

AGILITY_STAGED := oracle/_ref/libagilitycassie.a
ifeq ($(wildcard $(AGILITY)),)
AGILITY := $(AGILITY_STAGED)
endif
# Neither copy of the archive here: its 25 entry points are linked as stand-ins that print which block is missing and abort.
# Only the reference's host-side API needs the blocks (cassie_sim_*, cassie_batch_* / step_pd, the state estimator); the
# physics API (phys_*: Model / Batch) and everything on the device do not, and run as usual.  The library exports
# cassie_agility_blocks_absent so that a caller can tell such a build.  AGILITY_STAMP records which of the two the product
# was linked with, so that it is relinked whenever that changes (whatever the files' times).
AGILITY_ABSENT := $(OBJD)/agility_absent.o
AGILITY_SYMS := cassie_core_sim_alloc cassie_core_sim_copy cassie_core_sim_free cassie_core_sim_setup cassie_core_sim_step \
                pd_input_alloc pd_input_copy pd_input_free pd_input_setup pd_input_step \
                state_output_alloc state_output_copy state_output_free state_output_setup state_output_step \
                pack_cassie_in_t pack_cassie_out_t pack_cassie_user_in_t pack_pd_in_t pack_state_out_t \
                unpack_cassie_in_t unpack_cassie_out_t unpack_cassie_user_in_t unpack_pd_in_t unpack_state_out_t
AGILITY_STAMP := $(OBJD)/agility_link
ifneq ($(wildcard $(AGILITY)),)
AGILITY_LINK := -Wl,--whole-archive $(AGILITY) -Wl,--no-whole-archive
AGILITY_DEPS := $(AGILITY)
else
AGILITY_LINK := $(AGILITY_ABSENT)
AGILITY_DEPS := $(AGILITY_ABSENT)
endif

.PHONY: all product oracle emu wave_check models clean apps grad_resources opt_resources norm_resources draw_resources FORCE
all: product oracle emu apps
apps: $(PKG)/bin/cassiesim
product: $(PRODUCT)
oracle: oracle/libcassie_oracle.so
# (the wave checks' sources live in the test tree: a tree without them -- an older tests/ -- builds the rest as before)
WAVE_CHECK := $(if $(wildcard tests/device/wave_check.hip),tests/device/libwave_check.so)
emu: tests/emu/libcassie_emu.so $(WAVE_CHECK)
wave_check: tests/device/libwave_check.so

$(OBJD)/%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(wildcard include/*.h)
	@mkdir -p $(OBJD)
	g++ $(CXXFLAGS) -c $< -o $@
$(OBJD)/%.o: $(CSRC)/%.c $(wildcard $(CSRC)/*.h) $(wildcard include/*.h)
	@mkdir -p $(OBJD)
	gcc $(CFLAGS) -c $< -o $@
$(OBJD)/%.hip.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) $(wildcard $(CSRC)/*.inc) $(wildcard include/*.h)
	@mkdir -p $(OBJD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(AGILITY_STAMP): FORCE
	@mkdir -p $(OBJD)
	@echo '$(AGILITY_LINK)' | cmp -s - $@ || echo '$(AGILITY_LINK)' > $@

# (-z defs: an instantiation of the step kernel that phys_batch.hip names and no kernels_*.hip provides fails here, not at load time)
$(PRODUCT): $(OBJS) $(AGILITY_DEPS) $(AGILITY_STAMP)
	@test -f $(AGILITY) || echo "WARNING: no Agility archive (neither $(AGILITY) nor the reference's): linking stand-ins that abort when" \
	    "called; the reference's host-side API (cassie_sim_*, cassie_batch_*) is unusable in this build" >&2
	@mkdir -p $(LIBD)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,-z,defs -o $@ $(OBJS) $(AGILITY_LINK) -lm -lpthread

$(AGILITY_ABSENT):
	@mkdir -p $(OBJD)
	@{ echo '#include <stdio.h>'; echo '#include <stdlib.h>'; \
	   echo 'const int cassie_agility_blocks_absent = 1;'; \
	   printf '%s\n' 'static void absent(const char *f) { fprintf(stderr, "libcassiemujoco: %s belongs to the closed Agility library, which this build was linked without\n", f); abort(); }'; \
	   for f in $(AGILITY_SYMS); do echo "void $$f(void) { absent(\"$$f\"); }"; done; } > $(OBJD)/agility_absent.c
	gcc $(CFLAGS) -c $(OBJD)/agility_absent.c -o $@

# the UDP lock-step server (reference example/cassiesim.c role) against the product library
$(PKG)/bin/cassiesim: $(PKG)/apps/cassiesim.c $(PRODUCT)
	@mkdir -p $(PKG)/bin
	gcc -O2 -std=gnu11 -Iinclude -I$(CSRC) $< -o $@ -L$(LIBD) -lcassiemujoco -Wl,-rpath,'$$ORIGIN/../lib' -lm

oracle/libcassie_oracle.so: oracle/cassie_oracle.c oracle/cassie_oracle.h $(CSRC)/cm_model.h
	gcc -O2 -std=gnu11 -fPIC -shared -fopenmp -I$(CSRC) -Ioracle oracle/cassie_oracle.c -o $@ -lm

# the wave emulator: the scheduler (emu_runtime), the step kernel (emu_step: the one unit that instantiates it, and most of the build
# time; emu_lean: its lean and profiled fast forms; emu_sums: the forms of launches that accumulate the step sums), the small kernels and probes (emu_kernels), the depth image (emu_depth, emu_depth_scene), the placed restarts (emu_placement), the range sensors (emu_rays), the bank of full states (emu_states), the probes (emu_probes), the observation rows (emu_obs), the reward rows (emu_rewards), the action rows (emu_actions), the task rows (emu_task), the event rows (emu_events), the policy rows (emu_policy), the rollout rows (emu_rollout), the gradient rows (emu_grad), the optimiser rows (emu_opt), the normaliser rows (emu_norm) and the draw rows (emu_draw), compiled in parallel.  Baseline x86-64, no
# -march, no FMA contraction: the emulator's bit-exactness rests on these flags
# (the emulator's sources live in the test tree too: an older tests/, whose emulator is one chain of .cpp files that include each other
# from emu_terrain.cpp down, builds as it did -- one translation unit)
# -DCK_SENSORS_BEHIND_J_HFIELD=1: the emulator's 32-dof bodies are all instantiated with FEAT_ALL, height-field code included, and the
# product keeps wave 1's sensor stage in front of the barrier J in its height-field forms (physics_kernel.h: sensors_behind_j) -- the
# emulator would never run the order the benchmark's kernel has.  With the switch its 32-dof two-wave forms all take the new order
# (tests/test_sensor_stage_behind_j.py); the old one stays covered by its 40-dof two-wave form and by the GPU suite.
EMU_FLAGS := -O2 -std=c++17 -fPIC -Itests/emu -I$(CSRC) -Itests/device -DCK_SENSORS_BEHIND_J_HFIELD=1
EMU_DEPS  := $(wildcard tests/emu/*.h) $(wildcard tests/device/wave_bodies.h) $(wildcard $(CSRC)/*.h) $(wildcard $(CSRC)/*.inc)
ifeq ($(wildcard tests/emu/emu_terrain.cpp),)
EMU_OBJS := $(OBJD)/emu/emu_runtime.o $(OBJD)/emu/emu_step.o $(OBJD)/emu/emu_kernels.o $(OBJD)/emu/emu_depth.o $(OBJD)/emu/emu_depth_scene.o \
            $(OBJD)/emu/emu_placement.o $(OBJD)/emu/emu_rays.o $(OBJD)/emu/emu_lean.o $(OBJD)/emu/emu_sums.o $(OBJD)/emu/emu_states.o \
            $(OBJD)/emu/emu_probes.o $(OBJD)/emu/emu_obs.o $(OBJD)/emu/emu_rewards.o $(OBJD)/emu/emu_actions.o $(OBJD)/emu/emu_task.o \
            $(OBJD)/emu/emu_events.o $(OBJD)/emu/emu_policy.o $(OBJD)/emu/emu_rollout.o $(OBJD)/emu/emu_grad.o $(OBJD)/emu/emu_opt.o $(OBJD)/emu/emu_norm.o \
            $(OBJD)/emu/emu_draw.o
$(OBJD)/emu/%.o: tests/emu/%.cpp $(EMU_DEPS)
	@mkdir -p $(OBJD)/emu
	g++ $(EMU_FLAGS) -c $< -o $@
tests/emu/libcassie_emu.so: $(EMU_OBJS)
	g++ -shared -Wl,-Bsymbolic $(EMU_OBJS) -o $@
else
tests/emu/libcassie_emu.so: $(wildcard tests/emu/*.cpp) $(EMU_DEPS)
	g++ $(EMU_FLAGS) -shared -Wl,-Bsymbolic tests/emu/emu_terrain.cpp -o $@
endif

# the wave primitives and the kernel's numerical helpers one at a time (tests/test_wave_primitives.py): the bodies of
# wave_bodies.h for gfx950, with the product's flags -- the emulator library above runs the same bodies
tests/device/libwave_check.so: tests/device/wave_check.hip tests/device/wave_bodies.h $(wildcard $(CSRC)/*.h) $(wildcard $(CSRC)/*.inc) $(wildcard include/*.h)
	$(HIPCC) $(HIPFLAGS) -Itests/device -shared -o $@ $<

# registers, scratch and LDS of the gradient rows' kernels (csrc/grad_kernels.h), cross-compiled with the product's flags
grad_resources:
	SMALL=grad bash tools/kernel_resources.sh

# the same of the optimiser rows' kernels (csrc/opt_kernels.h)
opt_resources:
	SMALL=opt bash tools/kernel_resources.sh

# the same of the normaliser rows' kernels (csrc/norm_kernels.h)
norm_resources:
	SMALL=norm bash tools/kernel_resources.sh

# the same of the draw rows' kernels (csrc/draw_kernels.h)
draw_resources:
	SMALL=draw bash tools/kernel_resources.sh

models: product
	python3 tools/make_models.py $(REF)/model models tests/golden

clean:
	rm -rf $(OBJD) $(PRODUCT) oracle/libcassie_oracle.so tests/emu/libcassie_emu.so tests/device/libwave_check.so
