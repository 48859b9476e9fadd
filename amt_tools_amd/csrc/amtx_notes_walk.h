// The event walk of the note decoders, in one place: notes.hip (binary rolls) and thrgrid.hip (probability maps cut per threshold pair)
// both instantiate it, so a row's events cannot differ between the two.
//
// One wave64 owns a (clip, key) row and scans it BACKWARDS in 64-frame chunks, lane l holding frame ch * 64 + l.  The caller says, per
// lane, whether its frame is an impulse (an onset starts here) and whether the key is active; a frame that is inactive or an impulse is a
// "stop".  Every impulse becomes the event {its frame, the first stop strictly behind it (the row's length when there is none)}, written
// in descending frame order; the walk's state is the first stop behind the current chunk and the number of events so far.
#pragma once

#include "amtx_kernels.h"

struct NotesWalk {
    int next_stop;              // first stop frame strictly after the current chunk
    int n;                      // events found so far (descending frame order); the first `cap` of them are stored
};

static __device__ __forceinline__ NotesWalk notes_walk_begin(int T) { return NotesWalk{T, 0}; }

// One chunk of one row.  `imp` and `active` are false on lanes behind the row's end (`valid` false).
static __device__ __forceinline__ void notes_walk_chunk(NotesWalk& w, int ch, int lane, bool valid, bool imp, bool active, int cap, int2* __restrict__ out) {
    const int t = ch * 64 + lane;
    const bool stop = valid && (!active || imp);
    const unsigned long long smask = __ballot(stop);
    const unsigned long long above = (lane == 63) ? 0ull : (smask >> (lane + 1));
    const int my_next = above ? (t + 1 + __builtin_ctzll(above)) : w.next_stop;
    const unsigned long long imask = __ballot(imp);
    if (imp) {
        // events of this chunk in descending frame order after those of later chunks
        const int higher = __builtin_popcountll(lane == 63 ? 0ull : (imask >> (lane + 1)));
        const int slot = w.n + higher;
        if (slot < cap) out[slot] = make_int2(t, my_next);
    }
    w.n += __builtin_popcountll(imask);
    if (smask) w.next_stop = ch * 64 + __builtin_ctzll(smask);
}
