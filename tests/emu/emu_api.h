/*
 * emu_api.h -- TEST-ONLY: what a call of the wave emulator's step entry points is handed, as plain C structs passed by pointer
 * (tests/emu_py.py mirrors them; emu_sizeof_api / emu_offsetof_api let it check the mirror).  Nothing is kept from one call to the
 * next: the settings hold for the call they come with.
 */
#ifndef CASSIE_EMU_API_H
#define CASSIE_EMU_API_H

#include "cm_model.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test parameters of a call; all zero (emu_settings_default: resume_grid 2, chunks 1) = one instantiation alone, one wave per env */
typedef struct {
    int two_waves;              /* the two-wave forms (wave 1 runs the mass-matrix stage group) */
    int fast_rows;              /* the row-capped fast instantiation ahead of the full one, as phys_batch.hip launches them */
    int inplace;                /* the two-wave fast kernel in its in-place form */
    int inplace_stay_rows;      /* PhysIO::inplace_stay_rows (0: one substep at a time) */
    int chunks;                 /* PhysIO::nchunk of the fast kernel's launch (<= 1: in one piece) */
    int resume_grid;            /* workgroups of the pass that walks the first hand-over list (<= 0: 1) */
    int wave_schedule;          /* 0: the waves take turns, one rendezvous each; 1: wave 0 runs whenever it can; 2: wave 1 does */
    int force_runtime_topology; /* ck::pick_family's generic_only */
    int force_guarded_pgs;      /* every PGS sweep through its guarded form */
    int poison_lds;             /* fill the env's LDS block with NaN patterns at the start of every launch ... */
    unsigned long poison_lo, poison_hi; /* ... bytes [lo, hi) of it (hi 0: to its end) */
    int skip_com_init;          /* reinstate the round-2 bug (the centre-of-mass rows' once-per-launch initialisation) */
    int producer_xcc;           /* the "XCD" a chunk says it ran on when it publishes (consumers run on 0) */
} emu_settings;

typedef struct {
    const cm_model_t *model;
    int nenv, nsub, integrate;
    /* PhysIO's arrays, [nenv] rows of the model's sizes; the optional ones may be null */
    double *qpos, *qvel, *qacc_warmstart, *time;
    const double *ctrl, *qfrc_applied, *xfrc_applied;
    double *qacc, *sensordata, *actuator_velocity;
    int *warn, *info;
    double *xpos, *xquat;
    const double *pd_ptarget, *pd_kp, *pd_kd;
    /* drive-level I/O (mode = CM_DRIVE_*; all pointers may be null when mode is 0) */
    int drive_mode;
    cm_drive_state_t *drive_state;
    const double *drive_cmd;
    double *meas;
    const double *pd_dtarget, *pd_torque;
    const cm_envparams_t *envparams;    /* [nenv] per-env parameter blocks, or null: the model's own */
    /* the height field: hfield_stride floats between the grids (0: one shared grid), hfield_index null (env e reads grid e) or [nenv]
     * indices into a bank of nterrain grids */
    const float *hfield;
    unsigned long hfield_stride;
    const int *hfield_index;
    int nterrain;
    emu_settings settings;
} emu_step_args;

/* what the call did: envs the fast instantiation handed over, envs the 63-row pass handed on to the 127-row pass, and the word a
 * consumer chunk sets when it finds its producer on another "XCD" (PhysIO::chunk_fault) */
typedef struct { int fast_bails, wide_envs, chunk_fault; } emu_step_result;

int emu_phys_run(const emu_step_args *args, emu_step_result *result);
/* phys_batch_derive: a forward pass with the read-out enabled (the state, ctrl and the shared height field of args), then the derive kernel */
int emu_derive(const emu_step_args *args, const int *ids, double *derived, double *qM, emu_step_result *result);

#ifdef __cplusplus
}
#endif
#endif
