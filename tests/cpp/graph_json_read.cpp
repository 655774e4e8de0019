// Test code, never linked into the product: the engine's graph reader (csrc/graph_json.h, what load_json parses
// with) behind a C entry, so that a Python test can compare the floats it wrote with the floats the reader
// sees, bit for bit.  Returns 0, 1 if the file does not open or parse, 2 if the arrays are too small.
#include <stdint.h>

#include <fstream>
#include <sstream>

#include "../../trg-planner_amd/csrc/graph_json.h"

extern "C" int graph_json_read(const char *path, int cap_nodes, int cap_edges, int32_t *n_nodes, int32_t *n_edges,
                               int32_t *id, float *pos, int32_t *state, int32_t *source, int32_t *target,
                               float *weight, float *dist) {
  std::ifstream f(path);
  if (!f) return 1;
  std::stringstream ss;
  ss << f.rdbuf();
  trg::GraphJson g;
  std::string err;
  if (!trg::parse_graph_json(ss.str(), g, err) || !trg::validate_graph_json(g, err)) return 1;
  *n_nodes = (int32_t)g.nodes.size();
  *n_edges = (int32_t)g.edges.size();
  if (g.nodes.size() > (size_t)cap_nodes || g.edges.size() > (size_t)cap_edges) return 2;
  for (size_t i = 0; i < g.nodes.size(); ++i) {
    id[i] = g.nodes[i].id;
    for (int q = 0; q < 3; ++q) pos[3 * i + q] = g.nodes[i].p[q];
    state[i] = g.nodes[i].state;
  }
  for (size_t k = 0; k < g.edges.size(); ++k) {
    source[k] = g.edges[k].s;
    target[k] = g.edges[k].t;
    weight[k] = g.edges[k].w;
    dist[k] = g.edges[k].d;
  }
  return 0;
}
