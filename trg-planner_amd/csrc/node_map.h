// node_map.h -- the node map of a retained field solve through one update_graph ("Refresh", and
// section 7, "Refresh across tiles"): for every node of the current graph the id it had in the retained solve's graph,
// -1 for a node made since.  Host code without the engine, so that a stand-alone program can check it
// (tests/cpp/node_map_check.cpp).
#pragma once

#include <cstddef>
#include <vector>

namespace trg {

// A map in one of three states.  A successful solve starts it as the identity (no vector is kept), update_graph
// composes it with cleanGraph's renumbering, and a new solve's start, a replaced graph, a reset and an update that
// fails leave none.
struct NodeMap {
  enum State { NONE, IDENTITY, EXPLICIT } state = NONE;
  std::vector<int> ids;  // EXPLICIT only
};

// `map` (IDENTITY or EXPLICIT, of a graph of `nodes_before` nodes) taken through an update whose cleanGraph kept, as
// node k, the pre-clean node last_new2old[k]: a pre-clean id from nodes_before on is a node made by this update.
inline void node_map_compose(NodeMap &map, const std::vector<int> &last_new2old, size_t nodes_before) {
  std::vector<int> out(last_new2old.size());
  for (size_t k = 0; k < out.size(); ++k) {
    const int pre = last_new2old[k];
    if (pre < 0 || (size_t)pre >= nodes_before) out[k] = -1;
    else if (map.state == NodeMap::IDENTITY) out[k] = pre;
    else out[k] = (size_t)pre < map.ids.size() ? map.ids[pre] : -1;
  }
  map.ids.swap(out);
  map.state = NodeMap::EXPLICIT;
}

}  // namespace trg
