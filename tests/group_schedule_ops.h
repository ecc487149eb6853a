/*
 * group_schedule_ops.h -- the three operations of nbody_amd/csrc/group_common.h as tests/group_schedule.c supplies them
 * (NB_GROUP_OPS_HEADER): every one first yields to the program's scheduler.  NB_GROUP_STORE is no operation of the statement:
 * it exists for the planted defects alone (a compression or a hook done by a plain store).
 */
#ifndef GROUP_SCHEDULE_OPS_H
#define GROUP_SCHEDULE_OPS_H

#include <stdint.h>

uint32_t gs_load(const uint32_t *p);
uint32_t gs_cas(uint32_t *p, uint32_t expected, uint32_t desired); /* returns what the word held before */
void gs_min(uint32_t *p, uint32_t v);
void gs_store(uint32_t *p, uint32_t v);

#define NB_GROUP_LOAD(p) gs_load((p))
#define NB_GROUP_CAS(p, expected, desired) gs_cas((p), (expected), (desired))
#define NB_GROUP_MIN(p, v) gs_min((p), (v))
#define NB_GROUP_STORE(p, v) gs_store((p), (v))

#endif /* GROUP_SCHEDULE_OPS_H */
