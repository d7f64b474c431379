// The device-resident optimizer record (CLV_OPTIM_STATE_BYTES of include/clover_hip.h): clv_optim_prep writes it,
// clv_adamw_step_dev and clv_grad_report read it.
#pragma once
#include "../../include/clover_hip.h"

// The clip coefficient, Adam's bias corrections and Adam's OWN step count t, which advances only on steps that are taken —
// the reference skips optimizer.step() on a non-finite gradient (mmcv_Fp16OptimizerHook.py:123-141), so its Adam
// state['step'] does not move there either — all without a host round trip.
struct OptimState {
    float coef;        // grad_scale * min(1, max_norm / (norm + 1e-6))
    float bc1;         // 1 - beta1^t
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float norm;        // global gradient norm of this step (after grad_scale), for logging
    int skip;          // 1: non-finite norm, leave parameters and moments alone
    int t;             // Adam steps taken so far
    int skipped;       // steps skipped so far
    float grad_loss_scale;  // the loss_scale the gradients of the last clv_optim_prep carried, BEFORE a dynamic scale moved
                            // (clv_grad_report mode 0 reports it; formerly padding, and 0 until the first prep ran)
    // The loss scaler (fp16_utils.py:285-389 LossScaler), also on the device: the backward's root gradient is multiplied by
    // loss_scale (read from here by the host graph), clv_optim_prep divides it out again and — in dynamic mode — moves it.
    float loss_scale;      // current scale; 0: no scaler in use (the caller folds any static scale into grad_scale)
    float scale_factor;    // dynamic: the factor the scale moves by (reference default 2)
    int scale_window;      // dynamic: overflow-free iterations before the scale grows (reference default 1000)
    int scale_iter;        // LossScaler.cur_iter
    int last_overflow;     // LossScaler.last_overflow_iter (host initialises it to -1)
    int dynamic;           // 1: LossScaler(mode='dynamic'); 0: static
    int pad2[2];
};
static_assert(sizeof(OptimState) == CLV_OPTIM_STATE_BYTES, "OptimState layout is part of the ABI");
