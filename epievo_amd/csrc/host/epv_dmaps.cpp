// epv_dmaps.cpp -- see epv_dmaps.hpp
#include "epv_dmaps.hpp"

#include <algorithm>
#include <fstream>
#include <stdexcept>

namespace epv {

namespace {
// e[p] &= e[p + step] over a string of W words (bits beyond it are zero); in place, ascending: word i reads words >= i
void and_down(std::vector<uint64_t> &e, uint32_t step) {
  const size_t W = e.size(), q = step >> 6;
  const uint32_t s = step & 63u;
  for (size_t i = 0; i < W; ++i) {
    const uint64_t a = i + q < W ? e[i + q] : 0u, b = i + q + 1u < W ? e[i + q + 1u] : 0u;
    e[i] &= s ? (a >> s) | (b << (64u - s)) : a;
  }
}
// d[p] |= d[p - step]; in place, descending: word i reads words <= i
void or_up(std::vector<uint64_t> &d, uint32_t step) {
  const size_t W = d.size(), q = step >> 6;
  const uint32_t s = step & 63u;
  for (size_t i = W; i-- > 0;) {
    const uint64_t a = i >= q ? d[i - q] : 0u, b = i >= q + 1u ? d[i - q - 1u] : 0u;
    d[i] |= s ? (a << s) | (b >> (64u - s)) : a;
  }
}
inline uint32_t bit_of(const uint64_t *x, uint64_t j) { return (uint32_t)((x[j >> 6] >> (j & 63u)) & 1u); }
// bits st .. st + nbits - 1 of x (which holds xbits bits) as a string of its own, spare bits zero
void slice(const uint64_t *x, uint64_t xbits, uint64_t st, uint64_t nbits, uint64_t *out) {
  const uint64_t xw = (xbits + 63u) / 64u, ow = (nbits + 63u) / 64u;
  const uint32_t s = (uint32_t)(st & 63u);
  for (uint64_t j = 0; j < ow; ++j) {
    const uint64_t i = (st >> 6) + j;
    const uint64_t a = i < xw ? x[i] : 0u, b = i + 1u < xw ? x[i + 1u] : 0u;
    out[j] = s ? (a >> s) | (b << (64u - s)) : a;
  }
  if (ow && (nbits & 63u)) out[ow - 1u] &= ~0ull >> (64u - (nbits & 63u));
}
}  // namespace

void check_domain_map_sizes(uint32_t K, const uint32_t *sizes, const char *who) {
  const std::string w(who);
  if (K < 1u || K > kDmapsMaxSizes) throw std::runtime_error(w + ": 1 .. 4 sizes");
  for (uint32_t k = 0; k < K; ++k) {
    if (sizes[k] < 1u || sizes[k] > kDmapsMaxSize) throw std::runtime_error(w + ": a size is 1 .. 1024");
    if (k && sizes[k] <= sizes[k - 1u]) throw std::runtime_error(w + ": the sizes are strictly increasing");
  }
}

void domain_map_members(const uint64_t *x, uint64_t nbits, uint32_t L, uint64_t *out) {
  if (L < 1u) throw std::runtime_error("domain_map_members: a size is at least 1");
  const size_t W = (size_t)((nbits + 63u) / 64u);
  std::vector<uint64_t> e(x, x + W);
  for (uint32_t a = 1u; a < L;) {   // erosion: a bit stays where a run of a ones starts
    const uint32_t step = std::min(a, L - a);
    and_down(e, step);
    a += step;
  }
  for (uint32_t b = 1u; b < L;) {   // dilation: every site of the L that follow such a start
    const uint32_t step = std::min(b, L - b);
    or_up(e, step);
    b += step;
  }
  std::copy(e.begin(), e.end(), out);   // (a run of L ones ends inside the string: no spare bit is set)
}

void domain_maps_part(uint32_t N, uint32_t K, const uint32_t *sizes, uint64_t cnt, const uint64_t *bits,
                      uint32_t *counts, uint64_t *edges) {
  check_domain_map_sizes(K, sizes, "domain_maps_part");
  const uint32_t E = dmaps_edge_bits(sizes[K - 1u]), EW = dmaps_edge_words(sizes[K - 1u]);
  if (cnt < E)
    throw std::runtime_error("domain_maps_part: the stretch holds " + std::to_string(cnt) + " sites, fewer than the " +
                             std::to_string(E) + " of an edge record");
  const uint64_t words = (cnt + 63u) / 64u;
  std::vector<uint64_t> m(words);
  for (uint32_t v = 0; v < N; ++v) {
    const uint64_t *row = bits + (uint64_t)v * words;
    for (uint32_t k = 0; k < K; ++k) {
      domain_map_members(row, cnt, sizes[k], m.data());
      uint32_t *out = counts + ((uint64_t)v * K + k) * cnt;
      for (uint64_t p = 0; p < cnt; ++p) out[p] += bit_of(m.data(), p);
    }
    if (EW) {
      slice(row, cnt, 0u, E, edges + (uint64_t)v * 2u * EW);
      slice(row, cnt, cnt - E, E, edges + (uint64_t)v * 2u * EW + EW);
    }
  }
}

uint64_t domain_maps_merge(uint64_t n_parts, uint32_t N, uint32_t K, const uint32_t *sizes, uint64_t samples,
                           const uint64_t *cnts, const uint32_t *const *counts, const uint64_t *const *edges,
                           uint32_t *out_counts, uint64_t *out_edges) {
  check_domain_map_sizes(K, sizes, "domain_maps_merge");
  if (!n_parts) throw std::runtime_error("domain_maps_merge: no parts");
  const uint32_t E = dmaps_edge_bits(sizes[K - 1u]), EW = dmaps_edge_words(sizes[K - 1u]);
  uint64_t total = 0;
  std::vector<uint64_t> first(n_parts);   // a part's first site in the union
  for (uint64_t p = 0; p < n_parts; ++p) {
    if (cnts[p] < E)
      throw std::runtime_error("domain_maps_merge: part " + std::to_string(p) + " holds " + std::to_string(cnts[p]) +
                               " sites, fewer than the " + std::to_string(E) +
                               " of an edge record: a run's membership would depend on three parts");
    first[p] = total;
    total += cnts[p];
  }
  for (uint64_t r = 0; r < (uint64_t)N * K; ++r)
    for (uint64_t p = 0; p < n_parts; ++p)
      std::copy(counts[p] + r * cnts[p], counts[p] + (r + 1u) * cnts[p], out_counts + r * total + first[p]);
  if (!EW) return total;
  const uint32_t JW = (2u * E + 63u) / 64u;
  std::vector<uint64_t> joint(JW), mj(JW), mt(EW), mh(EW);
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t v = 0; v < N; ++v) {
      const uint64_t at = (s * N + v) * 2u * EW;
      for (uint64_t p = 0; p + 1u < n_parts; ++p) {
        const uint64_t *tail = edges[p] + at + EW, *head = edges[p + 1u] + at;
        // tail | head: the E bits before the boundary, then the E bits after it
        std::fill(joint.begin(), joint.end(), 0u);
        for (uint32_t j = 0; j < EW; ++j) joint[j] = tail[j];
        for (uint32_t j = 0; j < EW; ++j) {
          const uint32_t q = (E >> 6) + j, sh = E & 63u;
          joint[q] |= head[j] << sh;
          if (sh && q + 1u < JW) joint[q + 1u] |= head[j] >> (64u - sh);
        }
        const uint64_t b = first[p + 1u];   // the first site after the boundary
        for (uint32_t k = 0; k < K; ++k) {
          domain_map_members(joint.data(), 2u * E, sizes[k], mj.data());
          domain_map_members(tail, E, sizes[k], mt.data());
          domain_map_members(head, E, sizes[k], mh.data());
          uint32_t *out = out_counts + ((uint64_t)v * K + k) * total;
          // what the boundary hid is 0 or 1 per cell, and zero but in the L_k - 1 cells on either side of it
          for (uint32_t j = 0; j < E; ++j) {
            out[b - E + j] += bit_of(mj.data(), j) - bit_of(mt.data(), j);
            out[b + j] += bit_of(mj.data(), (uint64_t)E + j) - bit_of(mh.data(), j);
          }
        }
      }
      std::copy(edges[0] + at, edges[0] + at + EW, out_edges + at);
      std::copy(edges[n_parts - 1u] + at + EW, edges[n_parts - 1u] + at + 2u * EW, out_edges + at + EW);
    }
  return total;
}

void domain_map_windows(uint32_t N, uint32_t K, uint64_t n, const uint32_t *counts, uint64_t W, uint64_t *sums) {
  if (!W) throw std::runtime_error("domain_map_windows: a window holds at least one site");
  const uint64_t nw = (n + W - 1u) / W;
  std::fill(sums, sums + (uint64_t)N * K * nw, 0u);
  for (uint64_t r = 0; r < (uint64_t)N * K; ++r)
    for (uint64_t p = 0; p < n; ++p) sums[r * nw + p / W] += counts[r * n + p];
}

void write_domain_maps(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_samples,
                       uint32_t state, const std::vector<uint32_t> &sizes, uint64_t n_sites, uint64_t W,
                       const uint64_t *sums) {
  if (!W) throw std::runtime_error("write_domain_maps: a window holds at least one site");
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  const size_t N = node_names.size(), K = sizes.size(), nw = (size_t)((n_sites + W - 1u) / W);
  out << "#samples\t" << n_samples << "\tstate\t" << state << "\tsizes";
  for (uint32_t L : sizes) out << '\t' << L;
  out << "\n#window\t" << W << "\tsites\t" << n_sites << '\n';
  for (size_t v = 0; v < N; ++v) {
    out << "NODE:" << node_names[v] << '\n';
    for (size_t w = 0; w < nw; ++w)
      for (size_t k = 0; k < K; ++k) out << sums[(v * K + k) * nw + w] << (k + 1u == K ? '\n' : '\t');
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

DomainMaps read_domain_maps(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad domain-maps file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("domain-maps file " + file + ": " + what); };
  auto fields = [](const std::string &line) {
    std::vector<std::string> f;
    size_t a = 0;
    for (;;) {
      const size_t t = line.find('\t', a);
      f.push_back(line.substr(a, t == std::string::npos ? t : t - a));
      if (t == std::string::npos) break;
      a = t + 1;
    }
    return f;
  };
  DomainMaps dm;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() < 6 || f[0] != "#samples" || f[2] != "state" || f[4] != "sizes") throw bad("bad header: " + line);
  dm.n_samples = std::stoull(f[1]);
  dm.state = (uint32_t)std::stoul(f[3]);
  for (size_t i = 5; i < f.size(); ++i) dm.sizes.push_back((uint32_t)std::stoul(f[i]));
  if (dm.state > 1u) throw bad("the state is 0 or 1: " + line);
  try {
    check_domain_map_sizes((uint32_t)dm.sizes.size(), dm.sizes.data(), "sizes");
  } catch (const std::exception &e) { throw bad(e.what()); }
  if (!std::getline(in, line)) throw bad("no window line");
  f = fields(line);
  if (f.size() != 4 || f[0] != "#window" || f[2] != "sites") throw bad("bad window line: " + line);
  dm.window = std::stoull(f[1]);
  dm.n_sites = std::stoull(f[3]);
  if (!dm.window) throw bad("a window holds at least one site");
  const size_t K = dm.sizes.size(), nw = (size_t)((dm.n_sites + dm.window - 1u) / dm.window);
  size_t next = nw;   // the window the next line of the current node holds (nw: the node is complete)
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    if (line.compare(0, 5, "NODE:") == 0) {
      if (next != nw) throw bad("a node without all its windows before: " + line);
      dm.node_names.push_back(line.substr(5));
      dm.sums.resize(dm.node_names.size() * K * nw, 0u);
      next = 0;
      continue;
    }
    if (dm.node_names.empty()) throw bad("a line before the first node: " + line);
    f = fields(line);
    if (next >= nw || f.size() != K) throw bad("bad window line: " + line);
    for (size_t k = 0; k < K; ++k) dm.sums[((dm.node_names.size() - 1u) * K + k) * nw + next] = std::stoull(f[k]);
    ++next;
  }
  if (next != nw) throw bad("the last node lacks a window");
  return dm;
}

}  // namespace epv
