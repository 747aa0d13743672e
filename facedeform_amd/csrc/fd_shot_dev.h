// fd_shot_dev.h -- the device side of fdsop_cook_shot: everything of it that needs HIP lives in fd_capi.hip behind these
// calls, so that fd_sop_host.cpp stays free of HIP.  Internal: not part of the C ABI (include/facedeform_hip.h).
//
// One fd_shot_dev per node.  It owns two streams -- `work` (builds and evaluations of the shot's batches, in stream order)
// and `copy` (the downloads) -- the control tables of the shot (the rest rig and every frame's deltas, ONE device block), the
// mesh's transported vectors, and two staging sets in HBM that the groups' evaluations write in turn: group g is downloaded
// from its set on `copy` while group g + 1 is built and evaluated into the other set on `work`.
#ifndef FD_SHOT_DEV_H
#define FD_SHOT_DEV_H

#include "../../include/facedeform_hip.h"

struct fd_shot_dev;

fd_shot_dev *fd_shot_dev_create(fd_ctx *engine);                 // the engine whose device-resident mesh (fd_mesh_set) is evaluated
void fd_shot_dev_destroy(fd_shot_dev *sd);                       // waits for both streams first
const char *fd_shot_dev_error(const fd_shot_dev *sd);
void *fd_shot_dev_work_stream(fd_shot_dev *sd);                  // hipStream_t for fd_batch_build_async

// rest (M x 3) and deltas (F x M x 3, frame-major) from host arrays: one device block, one upload on `work`
int fd_shot_dev_set_rig(fd_shot_dev *sd, const float *rest, const float *deltas, int M, int F);
const float *fd_shot_dev_rest(const fd_shot_dev *sd);
const float *fd_shot_dev_delta(const fd_shot_dev *sd, int frame);
// the mesh's own N / tangentu / tangentv (npoints x 3 each, any of them NULL) for the vector launches; all NULL: no transport
int fd_shot_dev_set_vectors(fd_shot_dev *sd, const float *N, const float *tu, const float *tv);
// Two staging sets for groups of up to `frames` frames (positions, fall-off when asked for, a slice per transported vector).
// Returns the group size that could be allocated -- `frames`, or a smaller one when memory is short (halved until it fits) --
// or 0 when not even one frame fits twice.
int fd_shot_dev_reserve(fd_shot_dev *sd, int frames, int want_falloff);
// Evaluate the batch's models on the engine's mesh into staging set `set` (0 / 1), one launch: fp64 != 0 takes the fp64
// shot calls, multilayer != 0 the multilayer ones; with vectors set (above) the matching *_vectors_* call.  Waits (on the
// host) for the set's previous download.  The fall-off slices are zeroed first where a gate can leave entries unwritten.
int fd_shot_dev_eval(fd_shot_dev *sd, fd_batch *batch, int set, int fp64, int multilayer, float radius2, float falloffrate);
// One context of the last fd_shot_dev_eval evaluated again, in fp64, over slot `slot` of the set (a frame of an fp32 group
// whose error estimate does not hold); the context is FD_EVAL_FP32 again afterwards.
int fd_shot_dev_eval_fp64_over(fd_shot_dev *sd, fd_ctx *ctx, int set, int slot, float radius2, float falloffrate);
// Enqueue, on `copy` and behind the set's evaluations, the download of slots [0, n) into the callers' arrays (tables of n
// host pointers; P_out required; the others NULL or with NULL entries to skip).  Slots with skip[i] != 0 are left out.
int fd_shot_dev_deliver(fd_shot_dev *sd, int set, int n, const unsigned char *skip, float *const *P_out, float *const *falloff,
                        float *const *N_out, float *const *tu_out, float *const *tv_out);
int fd_shot_dev_wait(fd_shot_dev *sd, int set);                  // host: the set's last download has arrived
// The sequential path's transport: the engine's CURRENT model (the one fdsop_cook just built and evaluated, in the precision
// it chose) carries the vectors set above into host arrays, through slot 0 of set 0.  Synchronous.
int fd_shot_dev_vectors_engine(fd_shot_dev *sd, float radius2, float falloffrate, float *N_out, float *tu_out, float *tv_out);

#endif
