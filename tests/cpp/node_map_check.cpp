// node_map_check.cpp -- a stand-alone check of trg-planner_amd/csrc/node_map.h, the one loop that takes both node
// maps (the single-engine field's and the tiled one's) through an update, built with -fsanitize=address,undefined by
// tests/test_tiled_refresh_cpu.py.  Test code only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "node_map.h"

using trg::NodeMap;

static void expect(const NodeMap &m, const std::vector<int> &want, const char *what) {
  if (m.state != NodeMap::EXPLICIT || m.ids != want) {
    std::printf("node map: %s differs\n", what);
    std::exit(1);
  }
}

int main() {
  // an identity over 5 nodes; the update keeps pre-clean nodes 0, 2, 4 and two it made itself (5, 6), renumbered
  NodeMap m;
  m.state = NodeMap::IDENTITY;
  trg::node_map_compose(m, {4, 6, 0, 5, 2}, 5);
  expect(m, {4, -1, 0, -1, 2}, "the identity through one update");
  // a second update over those 5 nodes: drops node 1, makes one node, keeps the rest in another order
  trg::node_map_compose(m, {3, 0, 5, 4, 2}, 5);
  expect(m, {-1, 4, -1, 2, 0}, "two updates");
  // an update that keeps nothing, then one that only makes nodes
  trg::node_map_compose(m, {}, 5);
  expect(m, {}, "an update that keeps nothing");
  trg::node_map_compose(m, {0, 1, 2}, 0);
  expect(m, {-1, -1, -1}, "only new nodes");
  // ids that no graph has: a negative pre-clean id, and one past a map shorter than nodes_before says
  NodeMap s;
  s.state = NodeMap::EXPLICIT;
  s.ids = {7, 8};
  trg::node_map_compose(s, {-3, 1, 2, 0}, 4);
  expect(s, {-1, 8, -1, 7}, "ids outside the map");
  // a large identity
  NodeMap big;
  big.state = NodeMap::IDENTITY;
  std::vector<int> keep;
  for (int i = 0; i < 100000; i += 3) keep.push_back(i);
  trg::node_map_compose(big, keep, 100000);
  expect(big, keep, "a large identity");
  std::printf("node map: ok\n");
  return 0;
}
