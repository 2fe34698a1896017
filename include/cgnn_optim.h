/* cgnn_optim.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): the optimizer entry whose hyper-parameters live on the device.  It is additive:
 * CGNN_ABI_VERSION stays 2, and cgnn_adam_step (cgnn.h) keeps its signature and its bits.
 *
 * cgnn_adam_step_dev is cgnn_adam_step (same jobs, same shared step counter, same `arrivals` word, same `advance`) with
 * the five hyper-parameters read from device memory WHEN THE LAUNCH RUNS instead of being passed by value when it is
 * issued -- so a launch recorded in a HIP graph follows a learning-rate schedule: the host rewrites the row between
 * replays with a stream-ordered copy and the replayed launch reads the new values.
 *   hyper      DEVICE pointer to one row of CGNN_ADAM_HYPER_STRIDE doubles, 8-byte aligned:
 *              {lr, beta1, beta2, eps, weight_decay, 0, 0, 0}.  Every workgroup reads the first five; the read is
 *              issued together with the read of the step counter (neither depends on the other).  Nothing in the
 *              launch writes the row.  From it the kernel forms what cgnn_adam_step forms from its arguments, with the
 *              same doubles and the same roundings: float(beta2), float(1 - beta1), float(1 - beta2),
 *              float(sqrt(1 - beta2^t)), float(lr / (1 - beta1^t)), float(eps), float(weight_decay); with equal
 *              values the two entries leave equal bits in param, exp_avg and exp_avg_sq.
 *   decoupled  0: L2 weight decay, g += weight_decay * p (torch.optim.Adam, what cgnn_adam_step does);
 *              1: torch.optim.AdamW: p <- p * float(1 - lr * weight_decay), the factor formed in double and rounded
 *              once, the product rounded to float; then the Adam update with the gradient untouched.
 * The values are NOT checked: the host entry cannot see them.  Whoever writes the row checks, before the upload, what
 * cgnn_adam_step checks (lr >= 0, 0 <= beta < 1, eps >= 0; connectome_gnn_amd.optim.check_hyper).  A NULL or
 * misaligned `hyper`, a `decoupled` other than 0 or 1, and everything cgnn_adam_step refuses about `jobs`, `step` and
 * `arrivals` return CGNN_EINVAL before any launch.  One launch on `stream`; no allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_OPTIM_H
#define CGNN_OPTIM_H

#include "cgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_ADAM_HYPER_STRIDE 8
int cgnn_adam_step_dev(const cgnn_adam_jobs* jobs, float* step, uint32_t* arrivals, int32_t advance,
                       const double* hyper, int32_t decoupled, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_OPTIM_H */
