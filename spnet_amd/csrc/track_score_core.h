// The tracking score: the parts that do not depend on where the arrays live.  The rule is stated beside the prototypes in
// spnet_hip.h ("Tracking score").  csrc/track_score.hip calls these from its match and identity kernels, one lane per row
// or per identity; tools/track_score_host_check.cpp calls them over exact-size heap arrays, with the lanes in a loop, under
// AddressSanitizer.  The match of a frame -- truth rows with an effective identity against predicted rows that are live with
// track > 0 -- is tracks_core.h's mutual best (mutual_choose_a / _b, mutual_partner), the linker's: nothing of it is here.
//
// EFFECTIVE IDENTITY.  eff(t, k) = ident[t][k] where truth row (t, k) is live, 1 <= ident <= M and no live row k' < k of
// the frame has the same ident; 0 otherwise.  So an identity has at most one row a frame, and an ident outside 1 .. M is
// never an index.
//
// THE WALK.  One identity g over its frames in time order, one step per frame in which it is present:
//   matched    ++ where the frame's match is a prediction index 0 .. Kp-1
//   switches   ++ where it is matched and the predicted track differs from that of g's previous matched frame
//   fragments  ++ where it is matched, an unmatched present frame lies between this and g's previous matched frame
//   first      the first matched frame, -1 for none
#pragma once
#include "tracks_core.h"

namespace track_score {

constexpr int MAX_M = 65536;
constexpr int STATS = 5;                             // present, matched, switches, fragments, first_matched_frame

TR_HD bool sizes_ok(long N, int Kt, int Kp) {
  return tracks::sizes_ok(N, Kt) && tracks::sizes_ok(N, Kp) && N * (long)Kt * Kp <= tracks::MAX_FLAT;
}
TR_HD bool idents_ok(int M) { return M >= 1 && M <= MAX_M; }

// The effective identity of row k of one frame.  ident and live hold the frame's Kt entries.
TR_HD int effective_ident(const int* ident, const unsigned char* live, int k, int M) {
  const int g = ident[k];
  if (!live[k] || g < 1 || g > M) return 0;
  for (int m = 0; m < k; ++m)
    if (live[m] && ident[m] == g) return 0;
  return g;
}

struct Walk {
  int present = 0, matched = 0, switches = 0, fragments = 0, first = -1;
  int last_track = 0;
  bool gap = false;                                  // an unmatched present frame since the last matched one
};

// One present frame t of the identity: m = its row's match entry, track_row = the predicted frame's Kp track entries.
TR_HD void walk_step(Walk& w, int t, int m, const int* track_row, int Kp) {
  ++w.present;
  if (m < 0 || m >= Kp) {
    w.gap = w.matched > 0;
    return;
  }
  const int tr = track_row[m];
  if (w.matched > 0 && tr != w.last_track) ++w.switches;
  if (w.gap) ++w.fragments;
  if (w.matched == 0) w.first = t;
  ++w.matched;
  w.last_track = tr;
  w.gap = false;
}

// Identity g over the frames t_first .. t_last (clamped into 0 .. N-1): eff int32 [N][Kt] holds the effective identities,
// match int32 [N][Kt], track int32 [N][Kp].  Writes out[0 .. 4].
TR_HD void ident_walk(const int* eff, const int* match, const int* track, long N, int Kt, int Kp, int g, long t_first,
                      long t_last, int* out) {
  Walk w;
  if (t_first < 0) t_first = 0;
  if (t_last > N - 1) t_last = N - 1;
  for (long t = t_first; t <= t_last; ++t) {
    const int* e = eff + t * Kt;
    for (int k = 0; k < Kt; ++k)
      if (e[k] == g) {                                // at most one row a frame
        walk_step(w, (int)t, match[t * Kt + k], track + t * Kp, Kp);
        break;
      }
  }
  out[0] = w.present; out[1] = w.matched; out[2] = w.switches; out[3] = w.fragments; out[4] = w.first;
}

}  // namespace track_score
