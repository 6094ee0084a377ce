// Workgroup order of the batched block substitution (kp_solve.hip: kp_trsm2_batch_kernel), host and device.
//
// A system's ncb workgroups (one per block of 16 right-hand sides) all read that system's factor L.  The dispatcher hands
// consecutive workgroup ids to the chip's KP_SOLVE_XCDS dies in turn, each with an L2 of its own: a grid whose x index is the
// column block spreads every system over all eight L2s, and each of them fetches every L.  Here the workgroups of equal
// id % KP_SOLVE_XCDS - one die's - take whole systems, a system's column blocks consecutively:
//   die x = id % 8, its k-th workgroup k = id / 8:  system 8 (k / ncb) + x, column block k % ncb.
// A last, partial round of nb % 8 systems leaves the dies x >= nb % 8 without one: the grid is padded to whole rounds
// (kp_solve_xcd_grid) and those ids map to no system (false); at most 7 ncb workgroups that return at once.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KP_XCD_HD __host__ __device__
#else
#define KP_XCD_HD
#endif

#define KP_SOLVE_XCDS 8

// workgroups to launch for nb systems of ncb column blocks
KP_XCD_HD inline unsigned kp_solve_xcd_grid(int ncb, int nb) {
  return (unsigned)ncb * KP_SOLVE_XCDS * (unsigned)((nb + KP_SOLVE_XCDS - 1) / KP_SOLVE_XCDS);
}

// flat workgroup id -> (system, column block); false: a padding id of the last round
KP_XCD_HD inline bool kp_solve_xcd_map(unsigned id, int ncb, int nb, int* system, int* cb) {
  const unsigned k = id / KP_SOLVE_XCDS;
  *system = (int)(k / (unsigned)ncb) * KP_SOLVE_XCDS + (int)(id % KP_SOLVE_XCDS);
  *cb = (int)(k % (unsigned)ncb);
  return *system < nb;
}
