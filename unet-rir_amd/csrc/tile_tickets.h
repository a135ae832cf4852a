// tile_tickets.h - run-time tile tickets of the persistent kernels (conv3x3p, conv3x3d, conv3x3s, upconv3x3q): which tile of its
// group a workgroup takes next is decided while the kernel runs.  Device-only, internal to csrc/.
//
// Why: with a fixed assignment a workgroup that cannot be placed at once - a CU held by another kernel: a collective beside
// the backward pass, a weight-gradient kernel of the side stream - leaves its tiles for a second round after everybody else
// has finished (measured with 32 of 256 CUs held: 1.6x the launch time).  With tickets the workgroups that do run share all
// tiles of their group.
//
// The host/device contract (sched_slot() in api.hip hands out one slot per stream, unetrir_reset_tile_tickets() clears them):
//   * a slot is 65 words: sched[0 .. 63] are 64 group counters (8 per XCD: a kernel's group is (XCD, channel tile) or the XCD
//     alone, its counter sched[xcd * 8 + g]), sched[64] counts the workgroups that have finished;
//   * a ticket is the value a returning atomic add leaves: tickets 0, 1, 2, ... of a group in the order they were drawn.  How
//     a ticket maps to a tile (ranges per XCD, conv3x3d's even/odd interleave, conv3x3s's segments) is the kernel's business;
//     a ticket at or past the group's tile count means "no more tiles";
//   * every workgroup stops drawing at its first ticket past the end, so it has drawn its last - failing - ticket before it
//     counts itself out; the LAST workgroup to leave clears all 65 words, and the next launch on the stream finds zeros.
//     Launches that share a slot are ordered by their stream;
//   * sched == nullptr (dyn_tiles = 0, or a grid that does not cover every XCD): no counters, ticket k of a workgroup is
//     first + k * step - the fixed assignment.
//
// Inside a workgroup thread 0 draws and the others learn the ticket through 4 words of LDS: words 0, 1 the first two tickets
// (drawn with ONE atomic: one round trip at start-up), from byte 8 the hand-over word(s) of the tickets drawn later.  A later
// ticket is drawn with an inline-asm returning atomic: the compiler's own atomic sequence waits vmcnt(0) on the spot, i.e. for
// every DMA and store in flight.  The kernel decides where the atomic's latency hides: TICKETS_DRAW early, then its own counted
// s_waitcnt vmcnt(N) - the atomic is one more entry of that queue - in front of TICKETS_HAND_OVER, and TICKETS_RECEIVE behind a
// barrier.
// All LDS traffic is inline asm too: an LDS access the compiler can see makes it drain the DMA queue first.
#pragma once
#include <stdint.h>

// Macros, not functions: the kernels' schedules are pinned instruction by instruction, and statements that reach a kernel through
// an inlined function come out in another order (see conv3x3_tile.h).  CTR: the group's counter (unsigned*), nullptr for the
// fixed assignment; LDS_: LDS byte address (uint32_t) of the workgroup's ticket words.

// thread 0: the first two tickets -> LDS words 0, 1 (plain stores; a barrier follows).  FIXED0, FIXED1: the fixed assignment's.
#define TICKETS_FIRST_TWO(CTR, WORDS, FIXED0, FIXED1) do {                                                                       \
    unsigned* tk = reinterpret_cast<unsigned*>(WORDS);                                                                           \
    if (CTR) { const unsigned t = __hip_atomic_fetch_add(CTR, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); tk[0] = t; tk[1] = t + 1; } \
    else { tk[0] = (FIXED0); tk[1] = (FIXED1); }                                                                                 \
} while (0)

// thread 0: draw the next ticket into TK (unsigned); it is valid behind the caller's vmcnt wait.  CTR_ADDR: CTR as uint64_t;
// FIXED: the fixed assignment's.
#define TICKETS_DRAW(TK, CTR, CTR_ADDR, FIXED) do {                                                                              \
    if (CTR) asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(TK) : "v"(CTR_ADDR), "v"(1u) : "memory");               \
    else TK = (FIXED);                                                                                                           \
} while (0)

// thread 0: leave ticket TK in the hand-over word at LDS byte address LDS_ + 8
#define TICKETS_HAND_OVER(LDS_, TK) asm volatile("ds_write_b32 %0, %1 offset:8" :: "v"(LDS_), "v"(TK) : "memory")

// everybody, behind a barrier that follows the hand-over: TK (unsigned, wave-uniform) = the ticket in that word
#define TICKETS_RECEIVE(TK, LDS_) do {                                                                                           \
    unsigned v;                                                                                                                  \
    asm volatile("ds_read_b32 %0, %1 offset:8" : "=v"(v) : "v"(LDS_));                                                           \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                           \
    TK = (unsigned)__builtin_amdgcn_readfirstlane((int)v);                                                                       \
} while (0)

// thread 0 of every workgroup of the launch, last thing: the last one to leave clears the slot for the next launch
#define TICKETS_LEAVE(SCHED) do {                                                                                                \
    const unsigned d = __hip_atomic_fetch_add((SCHED) + 64, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                      \
    if (d == gridDim.x - 1) {                                                                                                    \
        for (int i = 0; i < 65; ++i) __hip_atomic_store((SCHED) + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);            \
    }                                                                                                                            \
} while (0)
