// zone_sets.h -- the keep-out zone lists of a field solve ("Keep-out zones"): the argument
// checks of trg_engine_cost_field_zones, the byte compare that decides whether two lists share a slot of the edge-cost
// cache, and the record a retained solve keeps them in.  Host code without the engine, so that a stand-alone program
// can check it (tests/cpp/zone_sets_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trg_engine.h"

namespace trg {

static_assert(sizeof(TrgZone) == 3 * sizeof(float), "a zone list is compared and copied as bytes");

// the member of `z` that makes it no zone ("x", "y" or "r"), or nullptr: x and y finite, r a finite number >= 0
inline const char *zone_bad_member(const TrgZone &z) {
  if (!std::isfinite(z.x)) return "x";
  if (!std::isfinite(z.y)) return "y";
  if (!(z.r >= 0.0f) || std::isinf(z.r)) return "r";
  return nullptr;
}

// The lists of m fields, field k's being zones[zone_ptr[k] .. zone_ptr[k + 1]): zone_ptr from 0 and never descending,
// at most TRG_ZONES_MAX zones a field, every zone one.  -> true, or false with `why` naming the field (and the zone).
inline bool zone_sets_check(int32_t m, const int32_t *zone_ptr, const TrgZone *zones, std::string &why) {
  if (zone_ptr[0] != 0) {
    why = "zone_ptr[0] is " + std::to_string(zone_ptr[0]) + ", not 0";
    return false;
  }
  for (int32_t k = 0; k < m; ++k) {
    const long long n = (long long)zone_ptr[k + 1] - zone_ptr[k];
    if (n < 0) {
      why = "zone_ptr descends at field " + std::to_string(k) + " (" + std::to_string(zone_ptr[k]) + ", then " +
            std::to_string(zone_ptr[k + 1]) + ")";
      return false;
    }
    if (n > TRG_ZONES_MAX) {
      why = "field " + std::to_string(k) + " has " + std::to_string(n) + " zones (0.." + std::to_string(TRG_ZONES_MAX) +
            ")";
      return false;
    }
    if (n > 0 && !zones) {
      why = "field " + std::to_string(k) + " has zones and `zones` is null";
      return false;
    }
    for (int32_t j = zone_ptr[k]; j < zone_ptr[k + 1]; ++j)
      if (const char *bad = zone_bad_member(zones[j])) {
        why = std::string(bad) + " of zone " + std::to_string(j - zone_ptr[k]) + " of field " + std::to_string(k) +
              (bad[0] == 'r' ? " is negative or not finite" : " is not finite");
        return false;
      }
  }
  return true;
}

// two lists are one list iff they are the same bytes (so -0 and +0 differ: two slots with the same verdicts)
inline bool zone_list_equal(const TrgZone *a, size_t na, const TrgZone *b, size_t nb) {
  return na == nb && (na == 0 || memcmp(a, b, na * sizeof(TrgZone)) == 0);
}

// The lists of a solve, as the retained record keeps them and a refresh hands them to the next solve.
struct ZoneSets {
  std::vector<int32_t> ptr;    // m + 1, or empty: the solve had no zone lists
  std::vector<TrgZone> zones;  // ptr[m]
  bool empty() const { return ptr.empty(); }
  void assign(int32_t m, const int32_t *zone_ptr, const TrgZone *z) {
    ptr.assign(zone_ptr, zone_ptr + m + 1);
    zones.clear();
    if (ptr[m] > 0) zones.assign(z, z + ptr[m]);
  }
};

}  // namespace trg
