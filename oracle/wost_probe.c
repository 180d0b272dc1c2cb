/*
 * wost_probe.c -- the oracle's deterministic math functions, one call per array of arguments, so
 * that tests/test_device_math.py can compare them with a high-precision reference (on the CPU)
 * and with the device's functions bit for bit (tests/probe/wost_probe.hip, same function table).
 * TEST INFRASTRUCTURE ONLY.  Nothing is restated here: the static functions come in through
 * wost_detmath.h, the others are the oracle's exported ones.
 */
#include <stdint.h>
#include <string.h>

#include "wost_oracle.h"
#include "wost_detmath.h"

double wo_vm_proposal_r(float kappa);   /* wost_vmm.c */

enum {
    FN_SINCOS_2PI = 0,   /* f32 -> 2 f32 (cos, sin) */
    FN_LOGF = 1,         /* f32 -> f32 */
    FN_EXPF = 2,         /* f32 -> f32 */
    FN_SINCOSF = 3,      /* f32 -> 2 f32 (cos, sin) */
    FN_CBRT01 = 4,       /* f32 -> f32 */
    FN_COSPI_D = 5,      /* f64 -> f64 */
    FN_ACOS_D = 6,       /* f64 -> f64 */
    FN_LOG_D = 7,        /* f64 -> f64 */
    FN_PCG = 8,          /* 3 u64 (initstate, initseq, delta) -> 8 u64 */
    FN_PROPOSAL_R = 9    /* f32 -> f64 */
};

void wo_probe(int32_t fn, const void *in, int64_t n, void *out)
{
    const float *fi = (const float *)in;
    const double *di = (const double *)in;
    const uint64_t *ui = (const uint64_t *)in;
    float *fo = (float *)out;
    double *dout = (double *)out;
    uint64_t *uo = (uint64_t *)out;
    for (int64_t i = 0; i < n; ++i) {
        switch (fn) {
        case FN_SINCOS_2PI: wo_sincos_2pi(fi[i], &fo[2 * i], &fo[2 * i + 1]); break;
        case FN_LOGF: fo[i] = wo_logf(fi[i]); break;
        case FN_EXPF: fo[i] = wo_expf(fi[i]); break;
        case FN_SINCOSF: wo_sincosf(fi[i], &fo[2 * i], &fo[2 * i + 1]); break;
        case FN_CBRT01: fo[i] = cbrt01(fi[i]); break;
        case FN_COSPI_D: dout[i] = wo_cospi_d(di[i]); break;
        case FN_ACOS_D: dout[i] = wo_acos_d(di[i]); break;
        case FN_LOG_D: dout[i] = wo_log_d(di[i]); break;
        case FN_PCG: {
            wo_pcg r;
            wo_pcg_set_seed(&r, ui[3 * i], ui[3 * i + 1]);
            uo[8 * i + 0] = r.state;
            uo[8 * i + 1] = r.inc;
            uo[8 * i + 2] = wo_pcg_next_uint(&r);
            const float f = wo_pcg_next_float(&r);
            uint32_t fb;
            memcpy(&fb, &f, 4);
            uo[8 * i + 3] = fb;
            uo[8 * i + 4] = wo_double_to_bits(wo_pcg_next_double(&r));
            uo[8 * i + 5] = r.state;
            wo_pcg_advance(&r, (int64_t)ui[3 * i + 2]);
            uo[8 * i + 6] = r.state;
            /* the device's pcg_skip2 claims to equal two discarded draws */
            (void)wo_pcg_next_uint(&r);
            (void)wo_pcg_next_uint(&r);
            uo[8 * i + 7] = r.state;
            break;
        }
        case FN_PROPOSAL_R: dout[i] = wo_vm_proposal_r(fi[i]); break;
        default: break;
        }
    }
}
