// The tracker's instances and entry point with an appearance (mydet_track_frames_appear_f32): csrc/track.hip as a second
// translation unit, so that the instances without one compile alone, to the code they always were (see the note there).
#define MYDET_TRACK_APPEAR 1
#include "track.hip"
