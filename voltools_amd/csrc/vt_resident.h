// vt_resident.h -- the resident copies a handle builds lazily besides its plain one: one table, and the rules that decide which copies
// a build may evict.  Bookkeeping only, no HIP: vt_api.hip allocates, frees and launches as the table decides (alloc_lazy / release);
// tests/resident_policy_driver.cpp runs the rules on the host.  The rules:
//   * per-call pins: while a call is in progress (begin_call .. end_call) a copy it has touched or allocated is never a victim;
//     outside a call (vt_volume_set_max_resident, vt_volume_release_copies) nothing is pinned;
//   * fit first: under a budget, a copy that cannot fit beside the fixed part (the plain copy and the projection helper) and the pinned
//     copies is refused before anything is evicted;
//   * victims go least recently used first; an evicted buffer becomes the spare (counted as resident), which the next build of at
//     most 1/8 less takes over at its real size;
//   * the transient source of a build (the exchanged plain copy a relayout reads) is pinned but not counted while the build runs, and
//     is the first thing released afterwards if the handle is over budget (trim).
#pragma once
#include <cstdint>
#include <vector>

namespace vt {

enum LazyCopyId {
    kCopyT = 0,                                // axes 0 and 1 exchanged ([y][z][x], pitch P): rotations about axis 1
    kCopyR,                                    // transposed in-plane ([z][x][y], pitch Pr): in-plane maps near a quarter turn
    kCopyX,                                    // axes 0 and 2 exchanged ([x][y][z], pitch Px): rotations about axis 2
    kCopyXe,                                   // plain layout convolved along axis 2 with the cubic weights of fraction 0 (row kernel, cubic)
    kCopyQ0, kCopyQ1, kCopyQ2, kCopyQ3,        // plane-quad forms ([z/4][y][x][4]) of the orientations plain, T, R, X
    kCopyQe0, kCopyQe1, kCopyQe2, kCopyQe3,    // ... of the z-convolved volume (cubic launches with an integer axis-0 offset)
    kCopyTmpX,                                 // the exchanged result of an axis-2 launch, before it is turned back
#ifdef VT_LEGACY
    kCopyP0, kCopyP1, kCopyP2, kCopyP3,        // plane-pair forms of the four orientations (round 1's cubic marching kernel): test build only
#endif
    kCopyCount
};

struct LazyCopy {
    void* ptr = nullptr;
    uint64_t bytes = 0;                        // size of the allocation ptr holds (a reused spare may be larger than the build asked for)
    uint64_t used = 0;                         // use_clock of the call that last touched it
    int retry_in = 0;                          // calls to go before a copy that could not be allocated or built is attempted again
};

struct LazyCopies {
    LazyCopy copy[kCopyCount];
    void* spare = nullptr;                     // the buffer of the copy evicted last, kept for the next build of about its size (a sweep
    uint64_t spare_bytes = 0;                  // under a budget trades one orientation's copy for another's: no hipFree + hipMalloc per switch)
    uint64_t max_resident = 0;                 // bytes the handle may keep resident, fixed part included (0 = no limit)
    uint64_t use_clock = 0;                    // calls so far
    bool in_call = false;

    // What a decision let go of: the caller waits until no launch reads these buffers, then frees `bufs`.  `evicted`: copies moved out
    // of the table to stay inside the budget or after a failed allocation (their buffers went to the spare).
    struct Released {
        std::vector<void*> bufs;
        std::vector<int> evicted;
        bool empty() const { return bufs.empty() && evicted.empty(); }
    };

    void begin_call() { ++use_clock; in_call = true; }
    void end_call() { in_call = false; }
    void touch(int id) { copy[id].used = use_clock; }
    bool pinned(int id) const { return in_call && copy[id].ptr && copy[id].used == use_clock; }
    void record(int id, void* p, uint64_t bytes) { copy[id].ptr = p; copy[id].bytes = bytes; touch(id); }
    void* forget(int id) { void* p = copy[id].ptr; copy[id].ptr = nullptr; copy[id].bytes = 0; return p; }
    uint64_t held() const
    {
        uint64_t tot = spare_bytes;
        for (const LazyCopy& c : copy) tot += c.bytes;
        return tot;
    }
    bool spare_fits(uint64_t bytes) const { return spare && spare_bytes >= bytes && spare_bytes - bytes <= bytes / 8; }
    void drop_spare(Released& rel)
    {
        if (spare) rel.bufs.push_back(spare);
        spare = nullptr; spare_bytes = 0;
    }
    void evict(int id, Released& rel)
    {
        drop_spare(rel);
        spare_bytes = copy[id].bytes;
        spare = forget(id);
        rel.evicted.push_back(id);
    }
    bool evict_lru(Released& rel)              // false when every copy is pinned or absent
    {
        int victim = -1;
        for (int id = 0; id < kCopyCount; ++id)
            if (copy[id].ptr && !pinned(id) && (victim < 0 || copy[id].used < copy[victim].used)) victim = id;
        if (victim >= 0) evict(victim, rel);
        return victim >= 0;
    }

    // Under a budget: evict until a build of `bytes` for copy `id` fits (the spare, if the build can take it over, at its real size).
    // False -- and nothing changed -- when it cannot fit beside the fixed part and the pinned copies except `transient` (-1: none).
    bool make_room(int id, uint64_t bytes, uint64_t fixed, int transient, Released& rel)
    {
        if (!max_resident) return true;
        uint64_t pinned_bytes = 0;
        for (int i = 0; i < kCopyCount; ++i)
            if (i != id && i != transient && pinned(i)) pinned_bytes += copy[i].bytes;
        auto reuse = [&] { return spare_fits(bytes) && fixed + pinned_bytes + spare_bytes <= max_resident; };
        if (fixed + pinned_bytes + (reuse() ? spare_bytes : bytes) > max_resident) return false;
        for (;;) {
            const uint64_t now = fixed + held() - (transient >= 0 ? copy[transient].bytes : 0);
            if (reuse() ? now <= max_resident : now + bytes <= max_resident) return true;
            if (spare && !reuse()) drop_spare(rel);
            else if (!evict_lru(rel)) return false;            // (not reached: the fit check leaves an unpinned copy to evict)
        }
    }
    bool take_spare(int id, uint64_t bytes)
    {
        if (!spare_fits(bytes)) return false;
        record(id, spare, spare_bytes);
        spare = nullptr; spare_bytes = 0;
        return true;
    }
    // after a failed allocation: the spare first, then the least recently used unpinned copy; false when nothing is left
    bool free_some(Released& rel)
    {
        if (!spare) return evict_lru(rel);
        drop_spare(rel);
        return true;
    }
    // back inside the budget: `first` (the transient source of a build, -1: none) goes first, then the spare and unpinned copies
    void trim(uint64_t fixed, int first, Released& rel)
    {
        if (!max_resident) return;
        if (first >= 0 && copy[first].ptr && fixed + held() > max_resident) evict(first, rel);
        while (fixed + held() > max_resident) {
            if (spare) drop_spare(rel);
            else if (!evict_lru(rel)) break;                     // (the fixed part alone may exceed a tiny budget: it stays)
        }
    }
    // every copy and the spare, and their bytes; memory was returned, so a copy that did not fit may fit now
    uint64_t release_all(Released& rel)
    {
        const uint64_t freed = held();
        drop_spare(rel);
        for (int id = 0; id < kCopyCount; ++id)
            if (copy[id].ptr) rel.bufs.push_back(forget(id));
        clear_retries();
        return freed;
    }
    void clear_retries() { for (LazyCopy& c : copy) c.retry_in = 0; }
};

}  // namespace vt
