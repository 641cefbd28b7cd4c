/*
 * emu_runtime.h -- TEST-ONLY: what a kernel's entry point needs from the wave emulator (emu_runtime.cpp: the scheduler and the wv::
 * primitives of tests/emu/wave.h), and the step kernel's C++ entry point (emu_step.cpp: the one unit that instantiates it).
 */
#ifndef CASSIE_EMU_RUNTIME_H
#define CASSIE_EMU_RUNTIME_H

#include "emu_api.h"

namespace emu {

/* a launch: workgroups 0 .. grid - 1 of nwaves waves each, one after the other in launch order (wv::env_id() = the workgroup,
 * wv::grid_size() = grid) */
void run_grid(void (*body)(), int grid, int nwaves = 1);

/* the settings the scheduler and wave.h's hooks read (wave_schedule, force_guarded_pgs, poison_*, skip_com_init, producer_xcc), for
 * the lifetime of this object: the defaults again when it goes */
struct with_settings {
    explicit with_settings(const emu_settings &s);
    ~with_settings();
    with_settings(const with_settings &) = delete;
};

/* a stepping launch as phys_batch.hip makes it (ck::plan_step's passes, the forms by args.settings).  ext: PhysIO::ext, the read-out
 * of phys_batch_derive's forward pass -- which takes the 63-row instantiation alone whatever the settings but two_waves say */
int run_step(const emu_step_args &args, emu_step_result &result, cm_ext_t *ext = nullptr);

}  // namespace emu
#endif
