/*
 * oracle/ref_probe/standin/curand_kernel.h -- TEST INFRASTRUCTURE.
 *
 * A stand-in for cuRAND's device interface (curandState, curand_init, curand,
 * curand_uniform), written from its documented interface.  The generator is a
 * TAPE: raw 32-bit words the probe was given, handed out in order.  The probe
 * selects a tape (ref_tape_select) and the next curand_init binds its state to
 * it; seed, subsequence and offset are ignored (the reference seeds from
 * clock()).  curand_uniform maps a word as oracle/philox.h does,
 * x * 2^-32 + 2^-33 in float: cuRAND's documented (0, 1].
 * Reading past the end of a tape ends the program with status 3.
 */
#ifndef REF_PROBE_STANDIN_CURAND_KERNEL_H
#define REF_PROBE_STANDIN_CURAND_KERNEL_H

#include "cuda_runtime.h"

struct ref_tape {
    const uint32_t* words;
    uint64_t len, pos;
};
extern ref_tape g_ref_tape; /* the selected tape; defined in the probe */

inline void ref_tape_select(const uint32_t* words, uint64_t len)
{
    g_ref_tape.words = words;
    g_ref_tape.len = len;
    g_ref_tape.pos = 0;
}

struct curandStateXORWOW { ref_tape* tape; };
typedef curandStateXORWOW curandState;
typedef curandStateXORWOW curandState_t;

inline void curand_init(unsigned long long, unsigned long long, unsigned long long, curandState* state) { state->tape = &g_ref_tape; }

inline unsigned int curand(curandState* state)
{
    ref_tape* t = state->tape;
    if (t->pos >= t->len) {
        std::fprintf(stderr, "ref_probe: the tape ran out after %llu words\n", (unsigned long long)t->len);
        std::fflush(nullptr);
        std::_Exit(3);
    }
    return t->words[t->pos++];
}

inline float curand_uniform(curandState* state)
{
    return (float)curand(state) * 2.3283064365386963e-10f + 1.1641532182693481e-10f;
}

#endif
