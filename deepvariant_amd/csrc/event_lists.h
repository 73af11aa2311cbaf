// event_lists.h -- the counter's events of one interval as per-position lists, and the one rule both
// passes behind the counter (gvcf.hip, candidates.hip) need from them: read_alleles is a map keyed by
// read key, so of the events of one key at one position only the one stored last stands.
#ifndef DV_EVENT_LISTS_H_
#define DV_EVENT_LISTS_H_

#include "dv_internal.h"

namespace dv {

struct EventLists {
  const dv_allele_event* events;   // in any order
  const int32_t* read_key;         // [n_reads] read-key id per read; null = every read is its own key
  int32_t* head;                   // [len] 1 + the first event of the position's list, 0 = none (zeroed before linking)
  int32_t* next;                   // [n_events] 1 + the next event of the same position, 0 = end
};

__device__ __forceinline__ int32_t key_of(const EventLists& l, uint32_t read) {
  return l.read_key ? l.read_key[read] : static_cast<int32_t>(read);
}

// The host's order of one position's events is (read, read_offset): the larger one is stored later.
__device__ __forceinline__ bool stored_before(const dv_allele_event& a, const dv_allele_event& b) {
  return a.read < b.read || (a.read == b.read && a.read_offset < b.read_offset);
}

// Pushes event `e` on the list of its position (the counter emits positions inside the interval only).
__device__ __forceinline__ void link_event(const EventLists& l, uint32_t e) {
  l.next[e] = atomicExch(&l.head[l.events[e].position], static_cast<int32_t>(e + 1));
}

// Is `ev` (= events[e]) the last event of its read key at its position?  All events must be linked.
__device__ __forceinline__ bool event_stands(const EventLists& l, uint32_t e, const dv_allele_event& ev) {
  const int32_t key = key_of(l, ev.read);
  bool last = true;
  for (int32_t j = l.head[ev.position]; j != 0 && last; j = l.next[j - 1]) {
    const dv_allele_event o = l.events[j - 1];
    if (static_cast<uint32_t>(j - 1) == e || key_of(l, o.read) != key) continue;
    last = !stored_before(ev, o);
  }
  return last;
}

}  // namespace dv

#endif  // DV_EVENT_LISTS_H_
