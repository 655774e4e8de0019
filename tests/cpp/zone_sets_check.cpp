// zone_sets_check.cpp -- a stand-alone check of trg-planner_amd/csrc/zone_sets.h: the zone-list checks of
// trg_engine_cost_field_zones, the byte compare that decides a cache slot, and the retained record, built with
// -fsanitize=address,undefined by tests/test_zone_ref_cpu.py.  Test code only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "zone_sets.h"

using trg::ZoneSets;

static void fail(const char *what) {
  std::printf("zone sets: %s\n", what);
  std::exit(1);
}

static void refused(int32_t m, const std::vector<int32_t> &ptr, const std::vector<TrgZone> &z, const char *needle,
                    const char *what) {
  std::string why;
  if (trg::zone_sets_check(m, ptr.data(), z.empty() ? nullptr : z.data(), why)) fail(what);
  if (why.find(needle) == std::string::npos) {
    std::printf("zone sets: %s: \"%s\" lacks \"%s\"\n", what, why.c_str(), needle);
    std::exit(1);
  }
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  std::string why;
  // accepted: no zones at all, a point zone, r = -0, the full 256, an empty list between two others
  const std::vector<int32_t> none{0, 0, 0};
  if (!trg::zone_sets_check(2, none.data(), nullptr, why)) fail("two empty lists are refused");
  std::vector<TrgZone> full(TRG_ZONES_MAX, TrgZone{1.0f, -2.0f, 0.0f});
  full[7].r = -0.0f;
  const std::vector<int32_t> one{0, TRG_ZONES_MAX};
  if (!trg::zone_sets_check(1, one.data(), full.data(), why)) fail("256 zones are refused");
  const std::vector<int32_t> gap{0, 2, 2, 5};
  if (!trg::zone_sets_check(3, gap.data(), full.data(), why)) fail("an empty list between two others is refused");
  // refused, and the message names what and where
  full.push_back(TrgZone{0.0f, 0.0f, 1.0f});
  refused(1, {0, TRG_ZONES_MAX + 1}, full, "field 0 has 257 zones", "257 zones are accepted");
  refused(2, {1, 2, 3}, full, "zone_ptr[0] is 1", "a zone_ptr from 1 is accepted");
  refused(2, {0, 3, 2}, full, "descends at field 1", "a descending zone_ptr is accepted");
  refused(1, {0, 2}, {}, "`zones` is null", "a null zone array is accepted");
  const float bad_xy[] = {nan, inf, -inf};
  const float bad_r[] = {nan, inf, -inf, -1.0f, -std::numeric_limits<float>::denorm_min()};
  for (float v : bad_xy) {
    refused(2, {0, 1, 3}, {{0, 0, 1}, {0, 0, 1}, {v, 0, 1}}, "x of zone 1 of field 1", "a bad x is accepted");
    refused(2, {0, 1, 3}, {{0, 0, 1}, {0, v, 1}, {0, 0, 1}}, "y of zone 0 of field 1", "a bad y is accepted");
  }
  for (float v : bad_r) refused(1, {0, 3}, {{0, 0, 1}, {0, 0, 1}, {5, 5, v}}, "r of zone 2 of field 0", "a bad r is accepted");
  // the byte compare: equal lists, one bit of r, a prefix, two empty lists, -0 against +0
  std::vector<TrgZone> a{{1, 2, 3}, {4, 5, 6}}, b = a;
  if (!trg::zone_list_equal(a.data(), 2, b.data(), 2)) fail("equal lists differ");
  b[1].r = std::nextafterf(b[1].r, inf);
  if (trg::zone_list_equal(a.data(), 2, b.data(), 2)) fail("one bit of r is not seen");
  if (trg::zone_list_equal(a.data(), 2, a.data(), 1)) fail("a prefix equals the list");
  if (!trg::zone_list_equal(nullptr, 0, a.data(), 0)) fail("two empty lists differ");
  b = a;
  b[0].x = -0.0f;
  a[0].x = 0.0f;
  if (trg::zone_list_equal(a.data(), 2, b.data(), 2)) fail("-0 equals +0");
  // the retained record: a deep copy that outlives its source, re-assigned shorter
  ZoneSets keep;
  if (!keep.empty()) fail("a new record is not empty");
  {
    std::vector<int32_t> ptr{0, 2, 2, 3};
    std::vector<TrgZone> z{{1, 1, 1}, {2, 2, 2}, {3, 3, 3}};
    keep.assign(3, ptr.data(), z.data());
  }
  if (keep.empty() || keep.ptr != std::vector<int32_t>({0, 2, 2, 3}) || keep.zones.size() != 3 || keep.zones[2].r != 3.0f)
    fail("the record differs from what it was given");
  if (!trg::zone_sets_check(3, keep.ptr.data(), keep.zones.data(), why)) fail("the record is refused");
  keep.assign(2, none.data(), nullptr);
  if (keep.empty() || keep.ptr.size() != 3 || !keep.zones.empty()) fail("empty lists are not kept as lists");
  std::printf("zone sets: ok\n");
  return 0;
}
