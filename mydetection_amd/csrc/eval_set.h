// The checks every mydet_eval_* and mydet_mot_* entry point makes on a mydet_eval_set (include/mydet.h).  Host side only.
#pragma once
#include "mydet.h"

// Nothing is dereferenced: the pointers are device pointers.
static inline int eval_check_set(const mydet_eval_set *s) {
    if (!s || (s->rotated != 0 && s->rotated != 1)) return MYDET_E_BADARG;
    if (s->I < 1 || s->K < 1 || s->D < 0 || s->G < 0 || s->n_groups < 0 || s->n_pairs < 0 || s->max_dt < 0 || s->max_gt < 0) return MYDET_E_BADARG;
    if (s->I > 0x7fffffff / s->K || s->n_groups > s->I * s->K || s->D > 0x7fffffff || s->G > 0x7fffffff) return MYDET_E_BADARG;
    if (!s->dt_start || !s->gt_start) return MYDET_E_BADARG;
    if (s->n_groups > 0 && (!s->groups || !s->pair_start)) return MYDET_E_BADARG;
    if (s->D > 0 && (!s->dt_box || !s->dt_score || !s->dt_area)) return MYDET_E_BADARG;
    if (s->G > 0 && (!s->gt_box || !s->gt_area || !s->gt_flags)) return MYDET_E_BADARG;
    if (s->max_dt > s->D || s->max_gt > s->G || s->n_pairs > s->D * s->G) return MYDET_E_BADARG;
    if ((s->D > 0 || s->G > 0) && s->n_groups == 0) return MYDET_E_BADARG;
    if (s->max_gt > MYDET_EVAL_MAX_GT || s->max_dt > MYDET_EVAL_MAX_DT) return MYDET_E_UNSUPP;
    return 0;
}
