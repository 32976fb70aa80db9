// The checks every mydet_eval_*, mydet_mot_* and mydet_hota_* entry point makes on a mydet_eval_set, and the last two on a
// mydet_mot_set beside it (include/mydet.h).  Host side only.
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

// The same for a mydet_mot_set beside its mydet_eval_set: a bad argument is reported before a cap.
static inline int mot_check(const mydet_eval_set *s, const mydet_mot_set *m) {
    const int code = eval_check_set(s);
    if (code == MYDET_E_BADARG) return code;
    if (!m || m->S < 1 || m->S > s->I) return MYDET_E_BADARG;
    if (m->max_gt_ids < 0 || m->max_dt_ids < 0 || m->n_gt_ids < 0 || m->n_dt_ids < 0 || m->n_ov < 0) return MYDET_E_BADARG;
    if (m->n_gt_ids > s->G || m->n_dt_ids > s->D || m->max_gt_ids > m->n_gt_ids || m->max_dt_ids > m->n_dt_ids) return MYDET_E_BADARG;
    if ((double)m->n_ov > (double)m->n_gt_ids * (double)m->n_dt_ids) return MYDET_E_BADARG;
    if (!m->seq_start || !m->gt_id_start || !m->dt_id_start || !m->ov_start) return MYDET_E_BADARG;
    if ((s->G > 0 && !m->gt_id) || (s->D > 0 && !m->dt_id)) return MYDET_E_BADARG;
    if (code) return code;
    if (m->max_gt_ids > MYDET_MOT_MAX_IDS || m->max_dt_ids > MYDET_MOT_MAX_IDS) return MYDET_E_UNSUPP;
    return 0;
}
