// rc_event_plan.h -- where a row walk of k_null meets its next frame-shift event, on the event mask of a strand x frame (bit j of
// word j / 64: some sequence has z != 0 at codon site j), free of HIP: the kernel calls these (rc_null_kernel.h), and
// tools/verify_event_plan.cpp compiles the same text for the host and compares it with the loops it replaced, which loaded the
// mask's word at every question (tests/test_event_plan_cpu.py).
//
// The word a walk is in lives in a register pair (EventMask::word, wave-uniform in the kernel): the word of sites 0..63 is loaded once
// per strand x frame, so a frame of up to 64 sites -- every launch with staged codes at its default LDS budget -- never loads another
// and no walk waits for a scalar load to find its next event.  Longer frames reload at each 64-site boundary they cross, in either
// direction (a new row starts in front of where the last one ended).
#pragma once

#if defined(__HIPCC__)
#define RC_EVENT_D __device__ __forceinline__
#else
#define RC_EVENT_D inline
#endif

namespace rc {

struct EventMask {
  const unsigned long long *words;   // the strand x frame's mask, (sites + 63) / 64 words
  int at;                            // the word held
  unsigned long long word;
};

// sites > 0: word 0 exists
RC_EVENT_D EventMask event_mask_begin(const unsigned long long *words) { return EventMask{words, 0, words[0]}; }

// the mask's word of site j (0 <= j < sites)
RC_EVENT_D unsigned long long event_mask_word(EventMask &m, int j) {
  if (__builtin_expect((j >> 6) != m.at, 0)) { m.at = j >> 6; m.word = m.words[m.at]; }
  return m.word;
}

// is site j (0 <= j < sites) an event codon?
RC_EVENT_D bool event_at(EventMask &m, int j) { return ((event_mask_word(m, j) >> (j & 63)) & 1ull) != 0ull; }

// first site >= j and < end with an event, or end (end <= sites; j >= end: end)
RC_EVENT_D int event_next(EventMask &m, int j, int end) {
  while (j < end) {
    const unsigned long long rest = event_mask_word(m, j) >> (j & 63);
    if (rest) { const int e = j + __builtin_ctzll(rest); return e < end ? e : end; }
    j = (j | 63) + 1;
  }
  return end;
}

}  // namespace rc
