// The closed-form acquisition tail, per point in double whatever the storage type: ONE copy for hb_sgp_acq
// (csrc/sgp_predict_grad.hip, where the formulas are written out) and hb_gram_predict (csrc/gram_matvec.hip).
#ifndef HB_ACQ_TAIL_CUH
#define HB_ACQ_TAIL_CUH

#include "common.cuh"
#include "../../include/henbun_hip.h"

#define ACQ_NONE (-1)                 // no tail

struct AcqTail {
  int acq;       // HB_ACQ_* or ACQ_NONE
  int largest;
  double best, param, scale, var_floor;
};
struct AcqPoint {
  double val, a_mu, a_v;
};

__device__ __forceinline__ AcqPoint acq_point(const AcqTail& t, double mean, double var) {
  const double s = t.largest ? 1.0 : -1.0, kvar = t.scale * t.scale;
  const double mu = s * t.scale * mean, vraw = kvar * var;
  const bool clamped = vraw < t.var_floor;
  const double v = clamped ? t.var_floor : vraw, sg = sqrt(v);
  AcqPoint o;
  if (t.acq == HB_ACQ_UCB) {
    o.val = mu + t.param * sg;
    o.a_mu = 1.0;
    o.a_v = t.param / (2.0 * sg);
  } else {
    const double u = (mu - s * t.best - t.param) / sg;
    const double Phi = 0.5 * erfc(-u * 0.70710678118654752440), phi = 0.39894228040143267794 * exp(-0.5 * u * u);
    if (t.acq == HB_ACQ_EI) {
      o.val = sg * (u * Phi + phi);
      o.a_mu = Phi;
      o.a_v = phi / (2.0 * sg);
    } else {
      o.val = Phi;
      o.a_mu = phi / sg;
      o.a_v = -u * phi / (2.0 * v);
    }
  }
  if (clamped) o.a_v = 0.0;
  return o;
}

// The arg-max rule of hb_sgp_pathwise_argmax, hb_sgp_acq and hb_gram_predict lives in csrc/sgp_pathwise.cuh (pw_takes).
#endif
