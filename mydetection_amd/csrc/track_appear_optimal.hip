// The tracker's instances and entry point of the optimal assignment on the fused IoU-and-appearance cost
// (mydet_track_frames_appear_optimal_f32): csrc/track.hip as a third translation unit, so that every instance that was there
// before compiles as it did, to the code it always was (see the note there).
#define MYDET_TRACK_APPEAR 1
#define MYDET_TRACK_APPEAR_OPTIMAL 1
#include "track.hip"
