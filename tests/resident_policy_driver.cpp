// Host driver of the resident-copy rules (voltools_amd/csrc/vt_resident.h), built and run by tests/test_resident_policy.py.
// usage: resident_policy_driver <case>; exit status 0 when the case holds, 1 (with a message) when it does not.
#include "vt_resident.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using vt::LazyCopies;

namespace {

int failures = 0;
#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// fake device buffers: distinct addresses, never dereferenced
char arena[64];
void* buf(int i) { return arena + i; }

bool same(const LazyCopies& a, const LazyCopies& b)
{
    for (int i = 0; i < vt::kCopyCount; ++i)
        if (a.copy[i].ptr != b.copy[i].ptr || a.copy[i].bytes != b.copy[i].bytes || a.copy[i].used != b.copy[i].used ||
            a.copy[i].retry_in != b.copy[i].retry_in) return false;
    return a.spare == b.spare && a.spare_bytes == b.spare_bytes && a.max_resident == b.max_resident && a.use_clock == b.use_clock;
}

// alloc_lazy's budget step on the table: make room, take the spare or record a fresh buffer
bool build(LazyCopies& l, int id, uint64_t bytes, uint64_t fixed, int transient, void* fresh, LazyCopies::Released& rel)
{
    if (!l.make_room(id, bytes, fixed, transient, rel)) return false;
    if (!l.take_spare(id, bytes)) l.record(id, fresh, bytes);
    return true;
}

// The sequence behind the high-severity finding: on the axis-0 <-> 2 path the exchanged-result buffer is allocated first, then the
// exchanged plain copy is requested in the same call.  The sizes are those of a 96 x 100 x 104 handle (pitch 128 floats).
void case_axis2_sequence()
{
    const uint64_t plain = 96ull * 100 * 128 * 4;                 // 4.9 MB
    const uint64_t out = 96ull * 100 * 104 * 4;                   // 0.81 x plain
    const uint64_t xcopy = 104ull * 100 * 128 * 4;                // 1.08 x plain (rows of D = 96 pitched to 128)
    LazyCopies l;
    l.max_resident = plain * 26 / 10;
    // an earlier call left the X copy's quad form behind
    l.begin_call();
    l.record(vt::kCopyQ3, buf(1), plain);
    l.end_call();
    l.begin_call();
    LazyCopies::Released rel;
    CHECK(build(l, vt::kCopyTmpX, out, plain, -1, buf(2), rel));
    CHECK(l.copy[vt::kCopyTmpX].ptr == buf(2));
    CHECK(rel.evicted.size() == 1 && rel.evicted[0] == vt::kCopyQ3);        // the unpinned copy of the earlier call made room
    rel = LazyCopies::Released();
    const LazyCopies before = l;
    CHECK(!build(l, vt::kCopyX, xcopy, plain, -1, buf(3), rel));            // 1 + 0.81 + 1.08 > 2.6: refused ...
    CHECK(rel.empty() && same(l, before));                                  // ... and the pinned result buffer is still there
    CHECK(l.copy[vt::kCopyTmpX].ptr == buf(2) && l.copy[vt::kCopyTmpX].bytes == out);
    // the no-budget failure loop applies the same pins: only the spare can go, then nothing
    l.max_resident = 0;
    l.spare = buf(4); l.spare_bytes = 64;
    CHECK(l.free_some(rel));
    CHECK(rel.bufs.size() == 1 && rel.bufs[0] == buf(4) && rel.evicted.empty());
    rel = LazyCopies::Released();
    CHECK(!l.free_some(rel) && rel.empty() && l.copy[vt::kCopyTmpX].ptr == buf(2));
    l.end_call();
}

// A copy that can never fit changes nothing: entries, spare and stamps stay as they were.
void case_never_fits()
{
    const uint64_t plain = 1000;
    LazyCopies l;
    l.max_resident = 3000;
    l.begin_call(); l.record(vt::kCopyT, buf(1), 1000); l.end_call();
    l.begin_call(); l.record(vt::kCopyQ1, buf(2), 900); l.end_call();
    l.spare = buf(3); l.spare_bytes = 100;
    l.copy[vt::kCopyQe0].retry_in = 5;
    l.begin_call();
    const LazyCopies before = l;
    LazyCopies::Released rel;
    CHECK(!l.make_room(vt::kCopyQ0, 2001, plain, -1, rel));                 // plain + 2001 > 3000 even with every copy gone
    CHECK(rel.empty() && same(l, before));
    // ... and with a pinned copy, one that would fit beside the plain copy alone is refused just the same
    l.touch(vt::kCopyT);
    const LazyCopies pinned = l;
    CHECK(!l.make_room(vt::kCopyQ0, 1500, plain, -1, rel));
    CHECK(rel.empty() && same(l, pinned));
    l.end_call();
}

// Unpinned victims go least recently used first; each evicted buffer becomes the spare, and a spare the build cannot take is freed.
void case_lru_order()
{
    LazyCopies l;
    l.max_resident = 1000 + 4 * 500;
    const int ids[3] = {vt::kCopyQ2, vt::kCopyT, vt::kCopyXe};             // built in this order, one call each
    for (int i = 0; i < 3; ++i) { l.begin_call(); l.record(ids[i], buf(i + 1), 500); l.end_call(); }
    l.begin_call();
    l.touch(vt::kCopyQ2);                                                   // the oldest one is read again in this call: pinned
    LazyCopies::Released rel;
    CHECK(l.make_room(vt::kCopyQ0, 1400, 1000, -1, rel));                   // 1000 + 1500 + 1400 > 3000: two must go
    CHECK(rel.evicted.size() == 2 && rel.evicted[0] == vt::kCopyT && rel.evicted[1] == vt::kCopyXe);
    CHECK(rel.bufs.size() == 2 && rel.bufs[0] == buf(2) && rel.bufs[1] == buf(3));      // (500 bytes do not serve 1400)
    CHECK(!l.spare && l.copy[vt::kCopyQ2].ptr == buf(1) && 1000 + l.held() + 1400 <= l.max_resident);
    l.end_call();
}

// A reused spare is counted at its real size in the fit check and in the footprint.
void case_spare_real_size()
{
    const uint64_t plain = 1000;
    LazyCopies l;
    l.spare = buf(1); l.spare_bytes = 1100;                                 // 10 % larger than the request below: reusable
    l.max_resident = plain + 1050;
    l.begin_call();
    LazyCopies::Released rel;
    CHECK(l.make_room(vt::kCopyQ0, 1000, plain, -1, rel));                  // the spare cannot fit (2100 > 2050): a fresh 1000 can
    CHECK(rel.bufs.size() == 1 && rel.bufs[0] == buf(1) && !l.spare);
    CHECK(!l.take_spare(vt::kCopyQ0, 1000));
    l.record(vt::kCopyQ0, buf(2), 1000);
    CHECK(plain + l.held() <= l.max_resident);
    l.end_call();
    // with room for it, the spare is taken over and the entry records its real size
    LazyCopies m;
    m.spare = buf(1); m.spare_bytes = 1100;
    m.max_resident = plain + 1100;
    m.begin_call();
    rel = LazyCopies::Released();
    CHECK(m.make_room(vt::kCopyQ0, 1000, plain, -1, rel) && rel.empty());
    CHECK(m.take_spare(vt::kCopyQ0, 1000));
    CHECK(m.copy[vt::kCopyQ0].ptr == buf(1) && m.copy[vt::kCopyQ0].bytes == 1100 && !m.spare && m.spare_bytes == 0);
    CHECK(plain + m.held() == 2100 && plain + m.held() <= m.max_resident);
    // a second copy that would fit at its requested size beside 1000 but not beside the real 1100 is refused
    rel = LazyCopies::Released();
    m.max_resident = plain + 1100 + 900;
    CHECK(!m.make_room(vt::kCopyQ1, 950, plain, -1, rel) && rel.empty());
    m.end_call();
}

// The exchanged plain copy a relayout reads is pinned and not counted during the build, and released first afterwards.
void case_transient_source()
{
    const uint64_t plain = 1000;
    LazyCopies l;
    l.max_resident = plain + 2200;
    l.begin_call(); l.record(vt::kCopyQe0, buf(1), 1000); l.end_call();      // an older copy, unpinned
    l.begin_call();
    LazyCopies::Released rel;
    CHECK(build(l, vt::kCopyR, 1000, plain, -1, buf(2), rel));              // the source: plain + Qe0 + R = 3000 <= 3200
    CHECK(rel.empty());
    CHECK(build(l, vt::kCopyQ2, 1500, plain, vt::kCopyR, buf(3), rel));     // counted, R would make 3500: refused; not counted, Qe0 goes
    CHECK(rel.evicted.size() == 1 && rel.evicted[0] == vt::kCopyQe0 && rel.bufs.size() == 1 && rel.bufs[0] == buf(1));
    CHECK(l.copy[vt::kCopyR].ptr == buf(2) && !l.spare);
    rel = LazyCopies::Released();
    // during the build the handle holds plain + R + Q2 = 3500 > 3200; afterwards R goes first
    l.trim(plain, vt::kCopyR, rel);
    CHECK(rel.evicted.size() == 1 && rel.evicted[0] == vt::kCopyR && rel.bufs.size() == 1 && rel.bufs[0] == buf(2));
    CHECK(!l.copy[vt::kCopyR].ptr && l.copy[vt::kCopyQ2].ptr == buf(3) && plain + l.held() <= l.max_resident);
    l.end_call();
    // within the budget the source stays
    LazyCopies m;
    m.max_resident = plain + 2000;
    m.begin_call();
    rel = LazyCopies::Released();
    CHECK(build(m, vt::kCopyR, 1000, plain, -1, buf(2), rel));
    CHECK(build(m, vt::kCopyQ2, 1000, plain, vt::kCopyR, buf(3), rel) && rel.empty());
    m.trim(plain, vt::kCopyR, rel);
    CHECK(rel.empty() && m.copy[vt::kCopyR].ptr == buf(2));
    m.end_call();
}

// Outside a call nothing is pinned: a budget set between calls may evict what the last call used; release_all frees everything.
void case_outside_call()
{
    const uint64_t plain = 1000;
    LazyCopies l;
    l.begin_call();
    l.record(vt::kCopyX, buf(1), 1000);
    l.record(vt::kCopyTmpX, buf(2), 800);
    CHECK(l.pinned(vt::kCopyX) && l.pinned(vt::kCopyTmpX));
    l.end_call();
    CHECK(!l.pinned(vt::kCopyX) && !l.pinned(vt::kCopyTmpX));
    l.max_resident = plain;
    LazyCopies::Released rel;
    l.trim(plain, -1, rel);
    CHECK(rel.evicted.size() == 2 && !l.spare && l.held() == 0);
    CHECK(rel.bufs.size() == 2);
    rel = LazyCopies::Released();
    l.max_resident = 0;
    l.begin_call(); l.record(vt::kCopyQ0, buf(3), 700); l.end_call();
    l.spare = buf(4); l.spare_bytes = 300;
    l.copy[vt::kCopyQ1].retry_in = 64;
    CHECK(l.release_all(rel) == 1000 && rel.bufs.size() == 2 && rel.evicted.empty());
    CHECK(l.held() == 0 && l.copy[vt::kCopyQ1].retry_in == 0);
}

}  // namespace

int main(int argc, char** argv)
{
    struct { const char* name; void (*run)(); } cases[] = {
        {"axis2_sequence", case_axis2_sequence}, {"never_fits", case_never_fits}, {"lru_order", case_lru_order},
        {"spare_real_size", case_spare_real_size}, {"transient_source", case_transient_source}, {"outside_call", case_outside_call},
    };
    if (argc != 2) { std::fprintf(stderr, "usage: %s <case>\n", argv[0]); return 2; }
    for (auto& c : cases)
        if (std::strcmp(argv[1], c.name) == 0) {
            c.run();
            return failures ? 1 : 0;
        }
    std::fprintf(stderr, "unknown case %s\n", argv[1]);
    return 2;
}
