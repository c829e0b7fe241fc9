/*
 * slim_gpu_groups.h -- engine extensions of libslim.so: the figures of an evaluation per user group, from the one
 * scoring pass the evaluation makes anyway, and a model-selection grid that chooses its pairs on one group.
 * Included by slim_gpu.h; plain C types only.
 *
 * Groups.  Every user u of [0, nall) -- nall: the rows of the eval set's staged test matrix -- has a group
 * group_of_user[u] in [0, ngroups), or -1: no group.  Groups go by USER ID, never by position: on an eval set of
 * listed users (SLIMGPU_EvalSetCreateAt(.., users)) the user at position q is users[q], as for a filter's exclusion
 * rows and a candidate set's rows.  A user of group -1 still counts in the row of everybody.
 *
 * While groups are set, every evaluation on the eval set -- SLIMGPU_ModelEvaluate, SLIMGPU_ModelEvaluateAt(Filtered),
 * SLIMGPU_ModelEvaluateRanked(Filtered), SLIMGPU_ModelEvaluateCandidates, SLIMGPU_ModelEvaluateExposure -- also forms
 * one row of figures per cutoff and group; SLIMGPU_EvalSetLastGroupFigures hands them out.  Outputs, paths and stats
 * of the calls themselves are unchanged, and without groups nothing changes at all: no launch, no byte.
 *
 * THE CONTRACT.  Take group g with at least one evaluated member.  Row (g, k) equals, bit for bit, row k of the same
 * call on an eval set made by SLIMGPU_EvalSetCreateAt / SLIMGPU_EvalSetCreateRanked for exactly that group's
 * evaluated users, ascending, with the same filter, candidate set and cutoffs.  (Users are scored independently of
 * each other, and every evaluation ends in one record per position and cutoff; the records of a group are added in
 * position order with the arithmetic of the sum over everybody: float accumulators fed double terms.)  A group with
 * no evaluated member gives zeros.  Row ngroups is everybody: the call's own output.
 *
 * Worked example: an eval set over users (0, 3, 6, 9, 12), hence positions 0 .. 4; ngroups 3 and
 * group_of_user = [1, 0, 0, 2, 0, 0, -1, 0, 0, 1, 0, 0, 1].  The evaluated users have groups 1, 2, -1, 1, 1:
 *   SLIMGPU_GroupPartition: order = [0, 3, 4, 1], offsets = [0, 0, 3, 4]   (position 2, user 6, is in no group)
 *   members = [0, 3, 1, 5]
 *   row 0 is zeros; row 1 is the call's row on an eval set of users (0, 9, 12); row 2 that of user (3); row 3 the
 *   call's own output, over all five.
 *
 * How it is made: one kernel, one wavefront per (cutoff, group), which gathers the records of
 * order[offsets[g] .. offsets[g + 1]) 64 at a time and adds them in lane order; every record is read once per cutoff
 * whatever ngroups is.  The sum over everybody is one more wavefront per cutoff of the same launch, through the code
 * of the launch it stands in for.  From the second evaluation after the groups were set: no device allocation,
 * nothing host to device, device to host the call's own bytes plus 32 * ncutoffs * ngroups.
 *
 * SLIM_ERROR_INPUT with a SLIMGPU_LastError text and the eval set as it was: a group outside [-1, ngroups); ngroups
 * outside [1, SLIMGPU_MAX_GROUPS]; a null argument; bounds that do not ascend strictly or lie below 1, nbounds outside
 * [1, SLIMGPU_MAX_GROUPS - 1].
 *
 * Not built: per-group exposure (the counting kernel would need a row mask: SLIMGPU_ModelEvaluateExposure gives the
 * accuracy rows per group and the exposure of everybody), overlapping groupings in one pass, several GPUs,
 * slim_predict.
 */
#ifndef SLIM_AMD_SLIM_GPU_GROUPS_H_
#define SLIM_AMD_SLIM_GPU_GROUPS_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMGPU_MAX_GROUPS 1024

typedef struct slimgpu_evalset slimgpu_evalset_t; /* (slim_gpu_eval.h) */
typedef struct slimgpu_filter slimgpu_filter_t;   /* (slim_gpu_filter.h) */
typedef struct slimgpu_grid slimgpu_grid_t;       /* (slim_gpu_grid.h) */

/* group_of_user[nall]; the array is copied; a second call replaces the first */
int32_t SLIMGPU_EvalSetSetGroups(slimgpu_evalset_t *es, int32_t ngroups, const int32_t *group_of_user);
/* groups by history length: bounds[nbounds] ascend strictly and are >= 1; the group of user u is
   #{j : history_length(u) >= bounds[j]}, hence nbounds + 1 groups, group 0 with the shortest histories.  The length
   is the staged matrix's row length, read where it lies and classified on the device */
int32_t SLIMGPU_EvalSetSetHistoryBands(slimgpu_evalset_t *es, int32_t nbounds, const int32_t *bounds);
void SLIMGPU_EvalSetClearGroups(slimgpu_evalset_t *es);
/* members[ngroups + 1] or NULL: the evaluated positions of every group, then every evaluated position.
   SLIM_ERROR_INPUT when no groups are set */
int32_t SLIMGPU_EvalSetGroupInfo(const slimgpu_evalset_t *es, int32_t *ngroups, int32_t *members);
/* the group rows of the most recent evaluation on this eval set: metrics[(g * ncutoffs + k) * 4 .. +4) and
   nvalid[(g * ncutoffs + k) * 3 .. +3) for g in [0, ngroups]; row ngroups is the call's own output.
   SLIM_ERROR_INPUT when no groups are set, when no evaluation has run since they were set, or when ncutoffs
   differs from that evaluation's */
int32_t SLIMGPU_EvalSetLastGroupFigures(slimgpu_evalset_t *es, int32_t ncutoffs, double *metrics, int32_t *nvalid);
/* host only, no device: the definition in code (host_csr.cpp), and the one routine every device path goes through.
   A stable counting sort of the positions by the group of their user (users NULL: position q is user q):
   order[offsets[g] .. offsets[g + 1]) are the positions of group g, ascending; positions of group -1 are not
   listed.  order: [nsel]; offsets: [ngroups + 1] */
int32_t SLIMGPU_GroupPartition(int32_t nsel, const int32_t *users, int32_t nall, int32_t ngroups,
                               const int32_t *group_of_user, int32_t *order, int64_t *offsets);

/* ---- the model-selection grid (slim_gpu_grid.h) ---------------------------------------------------------------- */

/* After SLIMGPU_GridOpen and before the first solve: every pair is also evaluated per group (group_of_user over the
   rows the grid evaluates: min(rows of trn, rows of tst)).  select_group in [0, ngroups) or -1 (everybody) is kept
   for the caller's loop.  Needs the evaluation in HBM (slim_gpu_grid.h lists what that takes): a grid without it is
   SLIM_ERROR_INPUT here, and never evaluates everybody in place of the groups.  Combines with the stride, a filter,
   sampled negatives and the exposure slot */
int32_t SLIMGPU_GridSetGroups(slimgpu_grid_t *grid, int32_t ngroups, const int32_t *group_of_user,
                              int32_t select_group);
/* members[ngroups + 1] or NULL: the positions the grid evaluates per group, then all of them (the eval set's
   SLIMGPU_EvalSetGroupInfo: with a stride, of the strided users).  SLIM_ERROR_INPUT without groups */
int32_t SLIMGPU_GridGroupInfo(const slimgpu_grid_t *grid, int32_t *ngroups, int32_t *members);
/* the last pair's figures at the grid's nrcmds: metrics[ngroups + 1][4], nvalid[ngroups + 1][3].  A pair that could
   not be evaluated per group is SLIM_ERROR from SLIMGPU_GridSolve, and this call then refuses: it never hands out an
   earlier pair's rows */
int32_t SLIMGPU_GridLastGroups(slimgpu_grid_t *grid, double *metrics, int32_t *nvalid);

#define SLIMGPU_GROUP_CELL 9 /* l1, l2, HR, HR_head, HR_tail, ARHR, nvalid, nvalid_head, nvalid_tail */
/* Py_SLIM_MselectFiltered (filter NULL: Py_SLIM_Mselect) with groups.  A pair's line is followed by one line per
   group: group, members, HR, HR_head, HR_tail, ARHR, nvalid.  The eight best-pair outputs are chosen on the figures
   of select_group with the loop's comparison rule (a pair whose select_group has no valid user ends the loop with
   SLIM_ERROR, as a pair without valid users does, and slim_mselect ends there too); -1 chooses as
   Py_SLIM_MselectFiltered.  cells:
   [nl1 * nl2][ngroups + 1][SLIMGPU_GROUP_CELL] in the order the pairs are solved (row ngroups: everybody), or NULL */
int32_t Py_SLIM_MselectGrouped(slim_t *trnhandle, slim_t *tsthandle, int32_t *ioptions, double *doptions,
                               double *arrayl1, double *arrayl2, int32_t nl1, int32_t nl2, double *bestl1HR,
                               double *bestl2HR, double *bestHRHR, double *bestARHR, double *bestl1AR,
                               double *bestl2AR, double *bestHRAR, double *bestARAR, slimgpu_filter_t *filter,
                               int32_t ngroups, const int32_t *group_of_user, int32_t select_group, double *cells);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_GROUPS_H_ */
