// epv_io.cpp -- see epv_io.hpp
#include "epv_io.hpp"
#include "epv_domains.hpp"
#include "epv_model.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <iostream>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <sstream>
#include <stdexcept>

namespace epv {

namespace {

struct Node {
  std::string name;
  double len = 0.0;
  bool generated = false;   // the name was made up by name_missing
  std::vector<Node> child;
};

// One Newick sub-expression "(a,b)name:len" -> Node.  Follows the reference's
// conventions (PhyloTree.cpp:124-203): a representation without a comma is a leaf;
// the name runs from after the last ')' to the first ':' after it; a missing length
// is 0.0; the length text is handed to atof.
Node parse_node(const std::string &rep) {
  Node nd;
  const size_t last_paren = rep.find_last_of(')');
  const size_t tail = (last_paren == std::string::npos) ? 0 : last_paren + 1;
  const size_t colon = rep.find(':', tail);
  nd.name = rep.substr(tail, (colon == std::string::npos ? rep.size() : colon) - tail);
  nd.len = (colon == std::string::npos) ? 0.0 : std::atof(rep.c_str() + colon + 1);
  if (rep.find(',') == std::string::npos) return nd;  // leaf
  // split the top-level comma list between the outer parentheses
  const size_t first = (rep[0] == '(') ? 1 : 0;
  const std::string inner = rep.substr(first, last_paren - first);
  int depth = 0;
  size_t start = 0;
  for (size_t i = 0; i <= inner.size(); ++i) {
    if (i == inner.size() || (depth == 0 && inner[i] == ',')) {
      nd.child.push_back(parse_node(inner.substr(start, i - start)));
      start = i + 1;
    } else if (inner[i] == '(') {
      ++depth;
    } else if (inner[i] == ')') {
      --depth;
    }
  }
  return nd;
}

// PhyloTreePreorder.cpp:79-86: the counter is passed BY VALUE into the children, so
// unnamed siblings can share a generated name -- kept for drop-in fidelity.
void name_missing(Node &nd, size_t count) {
  if (nd.name.empty()) { nd.name = "node_" + std::to_string(count++); nd.generated = true; }
  for (Node &c : nd.child) name_missing(c, count);
}

uint32_t flatten(const Node &nd, Tree &t) {
  const size_t me = t.subtree_sizes.size();
  t.subtree_sizes.push_back(1);
  t.branches.push_back(nd.len);
  t.node_names.push_back(nd.name);
  t.name_generated.push_back(nd.generated);
  for (const Node &c : nd.child) t.subtree_sizes[me] += flatten(c, t);
  return t.subtree_sizes[me];
}

void newick_of(const Tree &t, int node, std::ostringstream &oss) {
  if (t.subtree_sizes[node] > 1) {
    oss << '(';
    bool first = true;
    for (uint32_t c = 1; c < t.subtree_sizes[node]; c += t.subtree_sizes[node + c]) {
      if (!first) oss << ',';
      first = false;
      newick_of(t, node + (int)c, oss);
    }
    oss << ')';
  }
  // each reference node formats through its own fresh ostringstream (default precision)
  std::ostringstream num;
  num << t.branches[node];
  // the mains print the tree they READ (names are generated on TreeHelper's private copy,
  // TreeHelper.cpp:43-46), so a node without a name in the input stays without one
  const bool gen = (size_t)node < t.name_generated.size() && t.name_generated[node];
  oss << (gen ? std::string() : t.node_names[node]) << ':' << num.str();
}

}  // namespace

Tree Tree::parse(const std::string &newick_in) {
  std::string rep;
  int balance = 0;
  for (char c : newick_in) {
    if (std::isspace((unsigned char)c)) continue;
    if (c == '(') ++balance;
    if (c == ')') --balance;
    rep.push_back(c);
  }
  if (balance != 0) throw std::runtime_error("Unbalanced parentheses in Newick format: " + newick_in);
  if (rep.empty()) throw std::runtime_error("bad tree format");
  if (rep.back() == ';') rep.pop_back();
  Node root = parse_node(rep);
  name_missing(root, 0);
  Tree t;
  flatten(root, t);
  t.parent_ids.assign(t.subtree_sizes.size(), 0);
  for (size_t i = 0; i < t.subtree_sizes.size(); ++i)
    for (uint32_t c = 1; c < t.subtree_sizes[i]; c += t.subtree_sizes[i + c])
      t.parent_ids[i + c] = (uint32_t)i;
  return t;
}

Tree Tree::read(const std::string &tree_file) {
  std::ifstream in(tree_file);
  if (!in) throw std::runtime_error("bad tree file: " + tree_file);
  std::string rep;
  char c;
  bool found_end = false;
  while (!found_end && in >> c) {
    rep += c;
    if (c == ';') found_end = true;
  }
  if (!found_end) throw std::runtime_error("bad tree file: " + tree_file);
  return parse(rep);
}

Tree Tree::single_branch(double evo_time) {
  Tree t;
  t.subtree_sizes = {2, 1};
  t.node_names = {"root", "leaf"};
  t.parent_ids = {0, 0};
  t.branches = {0.0, evo_time};
  return t;
}

std::string Tree::newick() const {
  std::ostringstream oss;
  newick_of(*this, 0, oss);
  oss << ';';
  return oss.str();
}

// ---- local_paths files are the EM driver's bulk IO: 4e6 rows (111 MB) at n = 1e6 on tree.nwk, read
// once and REWRITTEN EVERY ITERATION (epievo_est_params_histories.cpp:280-283).  Both directions
// run on all host cores: the file is cut at row boundaries, the pieces are parsed / formatted
// independently and land at their own offsets (pread / pwrite), byte for byte the rows the
// sequential code produced.  EPV_IO_THREADS overrides the thread count (1 = sequential).
namespace {

unsigned io_threads(uint64_t rows) {
  unsigned t = std::thread::hardware_concurrency();
  if (t == 0) t = 1;
  if (t > 16) t = 16;
  if (const char *e = std::getenv("EPV_IO_THREADS")) { const int v = std::atoi(e); if (v >= 1 && v <= 256) t = (unsigned)v; }
  if (rows < 65536) t = 1;
  return t;
}

template <class F>
void parallel_jobs(unsigned n_jobs, unsigned n_threads, F &&job) {
  if (n_threads <= 1 || n_jobs <= 1) { for (unsigned j = 0; j < n_jobs; ++j) job(j); return; }
  std::vector<std::string> errors(n_jobs);
  std::atomic<unsigned> next(0);
  auto worker = [&] {
    for (;;) {
      const unsigned j = next.fetch_add(1);
      if (j >= n_jobs) return;
      try { job(j); } catch (const std::exception &e) { errors[j] = e.what(); }
    }
  };
  std::vector<std::thread> th;
  struct Join { std::vector<std::thread> &t; ~Join() { for (auto &x : t) if (x.joinable()) x.join(); } } join{th};
  for (unsigned i = 0; i + 1 < std::min(n_threads, n_jobs); ++i) th.emplace_back(worker);
  worker();
  for (auto &x : th) x.join();
  for (const std::string &e : errors) if (!e.empty()) throw std::runtime_error(e);
}

struct RowChunk {           // what one piece of a node's rows parses to
  std::vector<uint8_t> init;
  std::vector<uint64_t> cnt;
  std::vector<double> jumps;
};

// rows [p, end) of one node ('\n' separated, the buffer is NUL terminated behind its last byte);
// tt_text / tot_time: the node's tot_time token and value, known from its first row
void parse_rows(const char *p, const char *end, const std::string &tt_text, double tot_time, const std::string &path_file,
                RowChunk &out) {
  while (p < end) {
    const char *eol = (const char *)std::memchr(p, '\n', (size_t)(end - p));
    if (!eol) eol = end;
    char *stop = nullptr;
    // fast path for the common row "<site>\t<0|1>\t<tot_time>\t[jumps...]": digits, one state
    // character, and a tot_time token that repeats the node's first one byte for byte (then its
    // value is known without another strtod)
    const char *q = p;
    while (*q >= '0' && *q <= '9') ++q;
    bool have_row = true;
    if (q != p && *q == '\t' && (q[1] == '0' || q[1] == '1') && q[2] == '\t' &&
        (size_t)(eol - (q + 3)) >= tt_text.size() && std::memcmp(q + 3, tt_text.data(), tt_text.size()) == 0 &&
        (q[3 + tt_text.size()] == '\t' || q + 3 + tt_text.size() == eol)) {
      out.init.push_back(q[1] == '1');
      p = q + 3 + tt_text.size();
    } else {
      std::strtoull(p, &stop, 10);  // site index (ignored, rows are in order)
      if (stop == p || stop > eol) { have_row = false; }      // blank line
      else {
        p = stop;
        const long is = std::strtol(p, &stop, 10);
        p = stop;
        while (*p == ' ' || *p == '\t') ++p;
        const double tt = std::strtod(p, &stop);
        if (tt != tot_time) throw std::runtime_error("paths of one node disagree on tot_time: " + path_file);
        p = stop;
        out.init.push_back(is != 0);
      }
    }
    if (have_row) {
      uint64_t c = 0;
      while (p < eol && (*p == '\t' || *p == ' ')) ++p;
      while (p < eol) {             // most rows end here: no jumps
        const double v = std::strtod(p, &stop);
        if (stop == p) break;
        out.jumps.push_back(v);
        ++c;
        p = stop;
        while (p < eol && (*p == '\t' || *p == ' ')) ++p;
      }
      out.cnt.push_back(c);
    }
    p = eol + 1;
  }
}

}  // namespace

FlatPaths read_local_paths(const std::string &path_file, std::vector<std::string> &node_names,
                           std::vector<double> &tot_times) {
  const int fd = ::open(path_file.c_str(), O_RDONLY);
  if (fd < 0) throw std::runtime_error("cannot read: " + path_file);
  struct Fd { int fd; ~Fd() { ::close(fd); } } guard{fd};
  struct stat st;
  if (::fstat(fd, &st) != 0) throw std::runtime_error("cannot read: " + path_file);
  const uint64_t size = (uint64_t)st.st_size;
  std::vector<char> text(size + 1);
  const unsigned T = io_threads(size / 32);
  {
    const unsigned pieces = std::max(1u, T);
    parallel_jobs(pieces, T, [&](unsigned j) {
      uint64_t lo = size * j / pieces, hi = size * (j + 1) / pieces;
      while (lo < hi) {
        const ssize_t k = ::pread(fd, text.data() + lo, (size_t)std::min<uint64_t>(hi - lo, (uint64_t)1 << 30), (off_t)lo);
        if (k <= 0) throw std::runtime_error("error reading: " + path_file);
        lo += (uint64_t)k;
      }
    });
  }
  text[size] = '\0';
  const char *base = text.data(), *fin = base + size;
  // the NODE lines: at the start of the file, and behind a newline
  std::vector<const char *> heads;
  {
    const unsigned pieces = std::max(1u, T);
    std::vector<std::vector<const char *>> found(pieces);
    parallel_jobs(pieces, T, [&](unsigned j) {
      const char *lo = base + size * j / pieces, *hi = base + size * (j + 1) / pieces;
      for (const char *p = lo; p < hi;) {
        const char *q = (const char *)std::memchr(p, 'N', (size_t)(hi - p));
        if (!q) break;
        if ((q == base || q[-1] == '\n') && fin - q > 4 && std::memcmp(q, "NODE", 4) == 0) found[j].push_back(q);
        p = q + 1;
      }
    });
    for (auto &v : found) heads.insert(heads.end(), v.begin(), v.end());
  }
  if (heads.empty()) throw std::runtime_error("bad paths file (no NODE line): " + path_file);
  {
    // anything before the first NODE line must be blank
    for (const char *p = base; p < heads[0]; ++p)
      if (*p != '\n' && *p != ' ' && *p != '\t' && *p != '\r')
        throw std::runtime_error("bad paths file (no NODE line): " + path_file);
  }
  const size_t N = heads.size();
  if (N < 2) throw std::runtime_error("bad paths file: " + path_file);
  struct NodeBlock { const char *rows, *end; std::string tt_text; double tot_time = 0.0; };
  std::vector<NodeBlock> nb(N);
  for (size_t b = 0; b < N; ++b) {
    const char *eol = (const char *)std::memchr(heads[b], '\n', (size_t)(fin - heads[b]));
    if (!eol) eol = fin;
    const char *colon = (const char *)std::memchr(heads[b], ':', (size_t)(eol - heads[b]));
    node_names.push_back(colon ? std::string(colon + 1, eol) : std::string(heads[b], eol));
    nb[b].rows = eol < fin ? eol + 1 : fin;
    nb[b].end = b + 1 < N ? heads[b + 1] : fin;
    // the node's tot_time token: third field of its first row
    const char *p = nb[b].rows;
    while (p < nb[b].end && (*p == '\n' || *p == '\r')) ++p;
    if (p < nb[b].end) {
      char *stop = nullptr;
      std::strtoull(p, &stop, 10);
      if (stop != p) {
        p = stop;
        std::strtol(p, &stop, 10);
        p = stop;
        while (*p == ' ' || *p == '\t') ++p;
        nb[b].tot_time = std::strtod(p, &stop);
        nb[b].tt_text.assign(p, (size_t)(stop - p));
      }
    }
  }
  // every node's rows in `pieces` chunks cut at row boundaries
  const unsigned pieces = std::max(1u, T);
  std::vector<RowChunk> chunks(N * pieces);
  parallel_jobs((unsigned)(N * pieces), T, [&](unsigned job) {
    const size_t b = job / pieces, j = job % pieces;
    const char *lo = nb[b].rows, *hi = nb[b].end;
    const uint64_t len = (uint64_t)(hi - lo);
    const char *a = lo + len * j / pieces, *z = lo + len * (j + 1) / pieces;
    auto align = [&](const char *p) {     // first row start at or behind p
      if (p <= lo) return lo;
      if (p >= hi) return hi;
      const char *q = (const char *)std::memchr(p - 1, '\n', (size_t)(hi - (p - 1)));
      return q ? q + 1 : hi;
    };
    a = align(a);
    z = align(z);
    if (a < z) parse_rows(a, z, nb[b].tt_text, nb[b].tot_time, path_file, chunks[job]);
  });
  FlatPaths fp;
  fp.n_nodes = (int)N;
  tot_times.assign(N, 0.0);
  const uint64_t B = N - 1;
  std::vector<uint64_t> rows_of(N, 0), jumps_of(N, 0);
  for (size_t b = 0; b < N; ++b)
    for (unsigned j = 0; j < pieces; ++j) { rows_of[b] += chunks[b * pieces + j].init.size(); jumps_of[b] += chunks[b * pieces + j].jumps.size(); }
  fp.n_sites = rows_of[1];
  uint64_t total_jumps = 0;
  for (size_t b = 1; b < N; ++b) {
    if (rows_of[b] != fp.n_sites) throw std::runtime_error("nodes have different numbers of sites: " + path_file);
    tot_times[b] = nb[b].tot_time;
    total_jumps += jumps_of[b];
  }
  fp.init.resize(B * fp.n_sites);
  fp.offsets.resize(B * fp.n_sites + 1);
  fp.jumps.resize(total_jumps);
  // where every chunk lands
  std::vector<uint64_t> row0(N * pieces, 0), jmp0(N * pieces, 0);
  {
    uint64_t r = 0, jj = 0;
    for (size_t b = 1; b < N; ++b)
      for (unsigned j = 0; j < pieces; ++j) {
        row0[b * pieces + j] = r; jmp0[b * pieces + j] = jj;
        r += chunks[b * pieces + j].init.size(); jj += chunks[b * pieces + j].jumps.size();
      }
  }
  parallel_jobs((unsigned)(N * pieces), T, [&](unsigned job) {
    if (job < pieces) return;     // the root's block has no rows
    const RowChunk &c = chunks[job];
    std::copy(c.init.begin(), c.init.end(), fp.init.begin() + row0[job]);
    std::copy(c.jumps.begin(), c.jumps.end(), fp.jumps.begin() + jmp0[job]);
    uint64_t off = jmp0[job];
    for (size_t i = 0; i < c.cnt.size(); ++i) { fp.offsets[row0[job] + i] = off; off += c.cnt[i]; }
  });
  fp.offsets[B * fp.n_sites] = total_jumps;
  return fp;
}

// The EM driver rewrites the whole local_paths file every iteration
// (epievo_est_params_histories.cpp:280-283): 4e6 lines at n = 1e6.  Lines are assembled
// by hand: the site index by a backwards itoa, the per-branch constant "\t<init>\t<tot_time>\t"
// from two prebuilt strings, and only actual jump times (5 % of the lines on tree.nwk) go through
// printf's %.17g -- which is what ostream precision(max_digits10) in the default float format
// prints (Path.cpp:62-71).  A node's rows are formatted in pieces on all cores and written at their
// offsets with pwrite.
void write_local_paths(const std::string &path_file, const std::vector<std::string> &node_names,
                       int n_nodes, uint64_t n_sites, const double *tot_times,
                       const uint8_t *init, const uint64_t *offsets, const double *jumps) {
  const int fd = ::open(path_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) throw std::runtime_error("bad output file: " + path_file);
  struct Fd { int fd; ~Fd() { if (fd >= 0) ::close(fd); } } guard{fd};
  auto put = [&](const char *p, uint64_t len, uint64_t at) {
    while (len) {
      const ssize_t k = ::pwrite(fd, p, (size_t)std::min<uint64_t>(len, (uint64_t)1 << 30), (off_t)at);
      if (k <= 0) throw std::runtime_error("error writing: " + path_file);
      p += k; len -= (uint64_t)k; at += (uint64_t)k;
    }
  };
  uint64_t at = 0;
  {
    const std::string head = "NODE:" + node_names[0] + "\n";
    put(head.data(), head.size(), at);
    at += head.size();
  }
  const unsigned T = io_threads(n_sites);
  const unsigned pieces = T;
  std::vector<std::vector<char>> buf(pieces);
  for (int b = 1; b < n_nodes; ++b) {
    const std::string head = "NODE:" + node_names[b] + "\n";
    put(head.data(), head.size(), at);
    at += head.size();
    char num0[64];
    std::string tail[2];
    for (int is = 0; is < 2; ++is) {
      std::snprintf(num0, sizeof num0, "\t%d\t%.17g\t", is, tot_times[b]);
      tail[is] = num0;
    }
    parallel_jobs(pieces, T, [&](unsigned j) {
      std::vector<char> &out = buf[j];
      out.clear();
      const uint64_t s_lo = n_sites * j / pieces, s_hi = n_sites * (j + 1) / pieces;
      const uint64_t e0 = (uint64_t)(b - 1) * n_sites;
      const uint64_t nj = offsets[e0 + s_hi] - offsets[e0 + s_lo];
      out.resize((s_hi - s_lo) * (22 + tail[0].size()) + nj * 26 + 16);   // upper bound: 20 digits, tail, '\n'; 25 chars per jump
      char *w = out.data();
      char num[64];
      for (uint64_t s = s_lo; s < s_hi; ++s) {
        const uint64_t e = e0 + s;
        char *p = num + sizeof num;
        uint64_t v = s;
        do { *--p = (char)('0' + v % 10); v /= 10; } while (v);
        const size_t nd = (size_t)(num + sizeof num - p);
        std::memcpy(w, p, nd);
        w += nd;
        const std::string &t = tail[init[e] ? 1 : 0];
        std::memcpy(w, t.data(), t.size());
        w += t.size();
        for (uint64_t q = offsets[e]; q < offsets[e + 1]; ++q) w += std::snprintf(w, 32, "%.17g\t", jumps[q]);
        *w++ = '\n';
      }
      out.resize((size_t)(w - out.data()));
    });
    std::vector<uint64_t> pos(pieces + 1, at);
    for (unsigned j = 0; j < pieces; ++j) pos[j + 1] = pos[j] + buf[j].size();
    parallel_jobs(pieces, T, [&](unsigned j) { put(buf[j].data(), buf[j].size(), pos[j]); });
    at = pos[pieces];
  }
  const int rc = ::close(fd);
  guard.fd = -1;
  if (rc != 0) throw std::runtime_error("error writing: " + path_file);
}

void read_states_file(const std::string &states_file, std::vector<std::string> &names,
                      std::vector<std::vector<uint8_t>> &states) {
  std::ifstream in(states_file);
  if (!in) throw std::runtime_error("cannot read states file: " + states_file);
  std::string line;
  std::getline(in, line);
  if (!line.empty() && line[0] == '#') line = line.substr(1);
  std::istringstream hs(line);
  std::string nm;
  while (hs >> nm) names.push_back(nm);
  states.assign(names.size(), {});
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    size_t site = 0;
    ls >> site;
    size_t k = 0;
    char v = 0;
    while (k < names.size() && ls >> v) states[k++].push_back(v == '1');
    if (k != names.size()) throw std::runtime_error("bad line in states file");
  }
}

void read_states_file_missing(const std::string &states_file, std::vector<std::string> &names,
                              std::vector<std::vector<uint8_t>> &states, std::vector<std::vector<uint8_t>> &missing) {
  std::ifstream in(states_file);
  if (!in) throw std::runtime_error("cannot read states file: " + states_file);
  std::string line;
  std::getline(in, line);
  if (!line.empty() && line[0] == '#') line = line.substr(1);
  std::istringstream hs(line);
  std::string nm;
  while (hs >> nm) names.push_back(nm);
  states.assign(names.size(), {});
  missing.assign(names.size(), {});
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    size_t site = 0;
    ls >> site;
    size_t k = 0;
    char v = 0;
    for (; k < names.size() && ls >> v; ++k) {
      const bool miss = v == 'N' || v == 'n';
      states[k].push_back(v == '1');
      missing[k].push_back(miss ? 1u : 0u);
    }
    if (k != names.size()) throw std::runtime_error("bad line in states file");
  }
}

std::vector<uint64_t> read_regions(const std::string &regions_file, uint64_t n_sites) {
  std::ifstream in(regions_file);
  if (!in) throw std::runtime_error("cannot read regions file: " + regions_file);
  std::vector<uint64_t> lengths;
  uint64_t total = 0, line_no = 0, last = 0;
  std::string line;
  while (std::getline(in, line)) {
    ++line_no;
    std::istringstream is(line);
    std::vector<std::string> fields;
    for (std::string f; is >> f;) fields.push_back(f);
    if (fields.empty() || fields[0][0] == '#') continue;
    const std::string where = regions_file + ", line " + std::to_string(line_no) + ": ";
    if (fields.size() != 2)
      throw std::runtime_error(where + "a region is `name n_sites`, found " + std::to_string(fields.size()) + " fields");
    long long m = 0;
    size_t used = 0;
    try {
      m = std::stoll(fields[1], &used);
    } catch (const std::exception &) {
      used = 0;
    }
    if (used != fields[1].size() || used == 0)
      throw std::runtime_error(where + "the number of sites of region " + fields[0] + " is not an integer: " + fields[1]);
    if (m < 3)
      throw std::runtime_error(where + "region " + fields[0] + " holds " + std::to_string(m) +
                               " sites, a region holds at least 3");
    total += (uint64_t)m;
    if (total > n_sites)
      throw std::runtime_error(where + "the regions up to " + fields[0] + " hold " + std::to_string(total) +
                               " sites, the paths hold " + std::to_string(n_sites));
    lengths.push_back((uint64_t)m);
    last = line_no;
  }
  if (total != n_sites)
    throw std::runtime_error(regions_file + ", line " + std::to_string(last) + ": the regions hold " + std::to_string(total) +
                             " sites in all, the paths hold " + std::to_string(n_sites));
  return lengths;
}

std::vector<uint8_t> unobserved_leaf_cells(const std::string &states_file, const Tree &th, const FlatPaths &paths,
                                           uint64_t &n_unobserved, uint64_t &n_leaf_cells) {
  std::vector<std::string> names;
  std::vector<std::vector<uint8_t>> states, missing;
  read_states_file_missing(states_file, names, states, missing);
  const uint64_t n = paths.n_sites, N = (uint64_t)th.n_nodes();
  std::vector<uint8_t> mask((N - 1u) * n, 0u);
  n_unobserved = n_leaf_cells = 0;
  for (uint64_t node = 1; node < N; ++node) {
    if (!th.is_leaf((int)node)) continue;   // (columns of internal nodes are not data: ignored)
    const std::string &leaf = th.node_names[node];
    const size_t k = std::find(names.begin(), names.end(), leaf) - names.begin();
    if (k == names.size()) throw std::runtime_error("states file " + states_file + " has no column for leaf " + leaf);
    if (states[k].size() != n)
      throw std::runtime_error("states file " + states_file + " has " + std::to_string(states[k].size()) +
                               " sites, the paths " + std::to_string(n));
    for (uint64_t s = 0; s < n; ++s) {
      const uint64_t e = (node - 1u) * n + s;
      if (missing[k][s]) {
        mask[e] = 1u;
        ++n_unobserved;
        continue;
      }
      const uint32_t end = paths.init[e] ^ (uint32_t)((paths.offsets[e + 1] - paths.offsets[e]) & 1u);
      if (end != states[k][s])
        throw std::runtime_error("states file " + states_file + ": leaf " + leaf + " at site " + std::to_string(s) +
                                 " is " + std::to_string(states[k][s]) + ", the input paths end in " +
                                 std::to_string(end));
    }
    n_leaf_cells += n;
  }
  return mask;
}

void read_leaf_probs_file(const std::string &probs_file, std::vector<std::string> &names,
                          std::vector<std::vector<float>> &probs) {
  std::ifstream in(probs_file);
  if (!in) throw std::runtime_error("cannot read leaf probabilities file: " + probs_file);
  std::string line;
  std::getline(in, line);
  if (!line.empty() && line[0] == '#') line = line.substr(1);
  std::istringstream hs(line);
  std::string nm;
  while (hs >> nm) names.push_back(nm);
  probs.assign(names.size(), {});
  std::string tok;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    size_t site = 0;
    ls >> site;
    size_t k = 0;
    for (; k < names.size() && ls >> tok; ++k) {
      float r = std::numeric_limits<float>::infinity();   // (what no valid token gives)
      if (tok == "N" || tok == "n") {
        r = 0.5f;
      } else {
        char *end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end != tok.c_str() && *end == '\0' && v >= 0.0 && v <= 1.0) r = (float)v;
      }
      probs[k].push_back(r);
    }
    if (k != names.size()) throw std::runtime_error("bad line in leaf probabilities file");
  }
}

std::vector<float> leaf_evidence_cells(const std::string &probs_file, const Tree &th, const FlatPaths &paths,
                                       uint64_t &n_evidence, uint64_t &n_leaf_cells) {
  std::vector<std::string> names;
  std::vector<std::vector<float>> probs;
  read_leaf_probs_file(probs_file, names, probs);
  const uint64_t n = paths.n_sites, N = (uint64_t)th.n_nodes();
  std::vector<float> table((N - 1u) * n, std::numeric_limits<float>::quiet_NaN());
  n_evidence = n_leaf_cells = 0;
  for (uint64_t node = 1; node < N; ++node) {
    if (!th.is_leaf((int)node)) continue;   // (columns of internal nodes are not data: ignored)
    const std::string &leaf = th.node_names[node];
    const size_t k = std::find(names.begin(), names.end(), leaf) - names.begin();
    if (k == names.size())
      throw std::runtime_error("leaf probabilities file " + probs_file + " has no column for leaf " + leaf);
    if (probs[k].size() != n)
      throw std::runtime_error("leaf probabilities file " + probs_file + " has " + std::to_string(probs[k].size()) +
                               " sites, the paths " + std::to_string(n));
    for (uint64_t s = 0; s < n; ++s) {
      const uint64_t e = (node - 1u) * n + s;
      const float r = probs[k][s];
      if (!(r >= 0.0f && r <= 1.0f))
        throw std::runtime_error("leaf probabilities file " + probs_file + ": leaf " + leaf + " at site " +
                                 std::to_string(s) + " is neither a probability in [0, 1] nor N");
      if (r != 0.0f && r != 1.0f) {
        table[e] = r;
        ++n_evidence;
        continue;
      }
      // exactly 0 or 1 is data: it stays pinned (no table entry) and must be what the paths hold
      const uint32_t end = paths.init[e] ^ (uint32_t)((paths.offsets[e + 1] - paths.offsets[e]) & 1u);
      if (end != (r == 1.0f ? 1u : 0u))
        throw std::runtime_error("leaf probabilities file " + probs_file + ": leaf " + leaf + " at site " +
                                 std::to_string(s) + " is " + std::to_string(r == 1.0f ? 1 : 0) +
                                 ", the input paths end in " + std::to_string(end));
    }
    n_leaf_cells += n;
  }
  return table;
}

}  // namespace epv

namespace epv {

void add_path_counts(const FlatPaths &paths, const double *tot_times, uint32_t n_points,
                     std::vector<uint32_t> &counts) {
  const uint64_t n = paths.n_sites, B = paths.n_nodes > 0 ? (uint64_t)paths.n_nodes - 1u : 0u;
  if (n_points < 2) throw std::runtime_error("the number of points must be at least 2");
  counts.resize(B * n * n_points, 0u);
  std::vector<double> t(n_points);
  for (uint64_t b = 0; b < B; ++b) {
    const double bin = tot_times[b + 1] / (n_points - 1);
    double curr_time = bin;
    t[0] = 0.0;
    for (uint32_t i = 1; i < n_points; ++i, curr_time += bin) t[i] = curr_time;
    for (uint64_t s = 0; s < n; ++s) {
      const uint64_t e = b * n + s;
      const double *j0 = paths.jumps.data() + paths.offsets[e], *j1 = paths.jumps.data() + paths.offsets[e + 1];
      const uint32_t init = paths.init[e];
      uint32_t *c = counts.data() + e * n_points;
      c[0] += init;
      for (uint32_t i = 1; i < n_points; ++i) {
        const size_t idx = std::lower_bound(j0, j1, t[i]) - j0;
        c[i] += (idx % 2 == 0) ? init : 1u - init;
      }
    }
  }
}

void write_path_average(const std::string &file, const std::vector<std::string> &node_names, int n_nodes,
                        uint64_t n_sites, uint32_t n_points, const double *branch_len, const uint32_t *counts,
                        uint64_t n_samples) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  const double ns = (double)n_samples;
  out << "NODE:" << node_names[0] << std::endl;
  for (int b = 1; b < n_nodes; ++b) {
    out << "NODE:" << node_names[b] << "\t" << branch_len[b] << std::endl;
    for (uint64_t s = 0; s < n_sites; ++s) {
      const uint32_t *c = counts + ((uint64_t)(b - 1) * n_sites + s) * n_points;
      out << (double)c[0] / ns;
      for (uint32_t i = 1; i < n_points; ++i) out << "\t" << (double)c[i] / ns;
      out << '\n';
    }
  }
  if (!out) throw std::runtime_error("error writing: " + file);
}

void write_branch_events(const std::string &file, const std::vector<std::string> &node_names, int n_nodes,
                         uint64_t n_windows, uint64_t window, const double *branch_len, const uint64_t *sums,
                         uint64_t n_samples) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  out << "#samples\t" << n_samples << "\twindow\t" << window << '\n';
  const uint64_t B = (uint64_t)n_nodes - 1u;
  for (int b = 1; b < n_nodes; ++b) {
    out << "NODE:" << node_names[b] << "\t" << branch_len[b] << '\n';
    for (uint64_t w = 0; w < n_windows; ++w) {
      out << w * window;
      for (uint64_t p = 0; p < 6u; ++p) out << "\t" << sums[(p * B + (uint64_t)(b - 1)) * n_windows + w];
      out << '\n';
    }
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

void write_mixing(const std::string &file, uint32_t max_lag, const uint64_t *words, uint64_t n_sites, uint64_t window,
                  const uint32_t *moved, const uint64_t *sums) {
  const uint32_t K = max_lag;
  const uint64_t samples = words[0], moved_pairs = words[1];
  if (!samples) throw std::runtime_error("the mixing diagnostics hold no sample");
  if (!window) throw std::runtime_error("a window holds at least one site");
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  out << "#epievo-mixing 1\nsamples " << samples << "\nmoved_pairs " << moved_pairs << "\nmax_lag " << K << "\npairs";
  for (uint32_t k = 1; k <= K; ++k) out << ' ' << words[1u + k];
  out << "\nwindow " << window << "\nfirst_window 0\n#window sites moved move_rate";
  for (uint32_t k = 1; k <= K; ++k) out << " rho_" << k;
  out << " tau\n";
  const double nan = std::numeric_limits<double>::quiet_NaN(), ns = (double)samples;
  auto num = [&out](double v) {
    char buf[40];
    std::snprintf(buf, sizeof buf, " %.17g", v);
    out << buf;
  };
  std::vector<double> csum(K + 1u), rho(K + 1u);
  for (uint64_t w = 0, lo = 0; lo < n_sites; ++w, lo += window) {
    const uint64_t hi = n_sites - lo < window ? n_sites : lo + window;
    uint64_t msum = 0;
    double vsum = 0.0;
    std::fill(csum.begin(), csum.end(), 0.0);
    for (uint64_t p = lo; p < hi; ++p) {
      msum += moved[p];
      const double mean = (double)sums[p] / ns, var = (double)sums[n_sites + p] / ns - mean * mean;
      vsum += var;
      for (uint32_t k = 1; k <= K; ++k)
        csum[k] += words[1u + k] ? (double)sums[(uint64_t)(1u + k) * n_sites + p] / (double)words[1u + k] - mean * mean : nan;
    }
    rho[0] = vsum > 0.0 ? 1.0 : nan;
    for (uint32_t k = 1; k <= K; ++k) rho[k] = vsum > 0.0 ? csum[k] / vsum : nan;
    // Geyer's initial positive sequence: G_m = rho[2 m] + rho[2 m + 1], G_0 always, then while G_m > 0
    double tau = -1.0;
    for (uint32_t m = 0; 2u * m + 1u <= K; ++m) {
      const double G = rho[2u * m] + rho[2u * m + 1u];
      if (m && !(G > 0.0)) break;
      tau += 2.0 * G;
    }
    if (!(vsum > 0.0)) tau = nan;
    out << w << ' ' << hi - lo << ' ' << msum;
    num(moved_pairs ? (double)msum / ((double)moved_pairs * (double)(hi - lo)) : nan);
    for (uint32_t k = 1; k <= K; ++k) num(rho[k]);
    num(tau);
    out << '\n';
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

void write_change_patterns(const std::string &file, const std::vector<std::string> &node_names,
                           const std::vector<uint32_t> &subtree_sizes, uint32_t n_rows, uint64_t n_sites,
                           uint64_t n_windows, uint64_t window, const uint64_t *sums, uint64_t n_samples) {
  const size_t N = subtree_sizes.size();
  std::vector<std::string> names = {"jumps_1", "jumps_2", "jumps_3", "jumps_4", "jumps_5", "jumps_6", "jumps_7plus",
                                    "one_branch", "parallel_gain", "parallel_loss", "gain_and_loss", "reverted_only"};
  for (size_t v = 1; v < N; ++v) names.push_back("sole_gain:" + node_names[v]);
  for (size_t v = 1; v < N; ++v) names.push_back("sole_loss:" + node_names[v]);
  for (size_t v = 1; v < N; ++v) if (subtree_sizes[v] > 1u) names.push_back("clade_changed:" + node_names[v]);
  if (names.size() != n_rows) throw std::runtime_error("change patterns: the rows do not belong to this tree");
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  out << "#samples\t" << n_samples << "\twindow\t" << window << "\tsites\t" << n_sites << '\n';
  out << "#rows";
  for (const std::string &s : names) out << "\t" << s;
  out << '\n';
  for (uint64_t w = 0; w < n_windows; ++w) {
    out << w * window;
    for (uint64_t r = 0; r < n_rows; ++r) out << "\t" << sums[r * n_windows + w];
    out << '\n';
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

void write_window_stats(const std::string &file, const std::vector<std::string> &node_names, int n_nodes,
                        uint64_t n_windows, uint64_t window, const double *branch_len, const int *scale_exp,
                        const int64_t *counts, uint64_t n_samples, const double *J, const double *D,
                        const std::array<double, 8> &rates) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  char buf[64];
  auto g17 = [&](double v) { std::snprintf(buf, sizeof buf, "%.17g", v); return buf; };
  out << "#samples\t" << n_samples << "\twindow\t" << window << '\n';
  const uint64_t B = (uint64_t)n_nodes - 1u;
  for (int b = 1; b < n_nodes; ++b) {
    out << "NODE:" << node_names[b] << "\t" << g17(branch_len[b]) << "\t" << scale_exp[b] << '\n';
    for (uint64_t w = 0; w < n_windows; ++w) {
      out << w * window;
      for (uint64_t c = 0; c < 16u; ++c) out << "\t" << counts[(w * B + (uint64_t)(b - 1)) * 16u + c];
      out << '\n';
    }
  }
  out << "NODE:all\n";
  for (uint64_t w = 0; w < n_windows; ++w) {
    out << w * window;
    for (uint64_t c = 0; c < 8u; ++c) {
      int64_t j = 0;
      for (uint64_t b = 0; b < B; ++b) j += counts[(w * B + b) * 16u + c];
      out << "\t" << j;
    }
    for (uint64_t c = 0; c < 8u; ++c) {
      double d = 0.0;
      for (uint64_t b = 0; b < B; ++b) d += D[(w * B + b) * 8u + c];
      out << "\t" << g17(d);
    }
    out << "\t" << g17(regional_rate_factor(n_nodes, J + w * B * 8u, D + w * B * 8u, rates)) << '\n';
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

WindowStats read_window_stats(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad window-statistics file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("window-statistics file " + file + ": " + what); };
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
  WindowStats ws;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() != 4 || f[0] != "#samples" || f[2] != "window") throw bad("bad header: " + line);
  ws.n_samples = std::stoull(f[1]);
  ws.window = std::stoull(f[3]);
  std::vector<std::vector<int64_t>> rows;   // the current node's windows
  std::vector<std::vector<std::vector<int64_t>>> nodes;
  bool in_all = false;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    f = fields(line);
    if (line.compare(0, 5, "NODE:") == 0) {
      if (in_all) throw bad("a node after NODE:all");
      if (!ws.node_names.empty()) nodes.push_back(rows);
      rows.clear();
      if (line == "NODE:all") { in_all = true; continue; }
      if (f.size() != 3) throw bad("bad node line: " + line);
      ws.node_names.push_back(f[0].substr(5));
      ws.branch_len.push_back(std::stod(f[1]));
      ws.scale_exp.push_back(std::stoi(f[2]));
    } else if (in_all) {
      if (f.size() != 18) throw bad("bad line in NODE:all: " + line);
      const uint64_t w = ws.factor.size();
      if (std::stoull(f[0]) != w * ws.window) throw bad("windows out of order: " + line);
      for (int c = 0; c < 8; ++c) ws.all_J.push_back(std::stoll(f[1 + c]));
      for (int c = 0; c < 8; ++c) ws.all_D.push_back(std::stod(f[9 + c]));
      ws.factor.push_back(std::strtod(f[17].c_str(), nullptr));   // (takes "nan")
    } else {
      if (ws.node_names.empty() || f.size() != 17) throw bad("bad window line: " + line);
      if (std::stoull(f[0]) != rows.size() * ws.window) throw bad("windows out of order: " + line);
      std::vector<int64_t> r(16);
      for (int c = 0; c < 16; ++c) r[c] = std::stoll(f[1 + c]);
      rows.push_back(r);
    }
  }
  if (!in_all) throw bad("no NODE:all block");
  const uint64_t B = ws.node_names.size();
  ws.n_windows = ws.factor.size();
  if (nodes.size() != B) throw bad("node blocks missing");
  ws.counts.assign(ws.n_windows * B * 16u, 0);
  for (uint64_t b = 0; b < B; ++b) {
    if (nodes[b].size() != ws.n_windows) throw bad("node " + ws.node_names[b] + " has another number of windows");
    for (uint64_t w = 0; w < ws.n_windows; ++w)
      std::copy(nodes[b][w].begin(), nodes[b][w].end(), ws.counts.begin() + (w * B + b) * 16u);
  }
  return ws;
}

void write_lineage_origins(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_rows,
                           const uint32_t *leaf_node, const uint32_t *branch_node, uint64_t n_windows, uint64_t window,
                           int scale_exp, const uint64_t *origin, const uint64_t *age, uint64_t n_samples) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  out << "#samples\t" << n_samples << "\twindow\t" << window << "\tscale_exp\t" << scale_exp << '\n';
  for (uint64_t r = 0; r < n_rows; ++r)
    out << "#row\t" << r << "\t" << node_names.at(leaf_node[r]) << "\t" << node_names.at(branch_node[r]) << '\n';
  uint64_t leaf = 0;
  for (uint64_t r0 = 0; r0 < n_rows; ++leaf) {
    uint64_t r1 = r0;
    while (r1 < n_rows && branch_node[r1] != 0u) ++r1;   // the root row ends a leaf's rows
    if (r1 == n_rows) throw std::runtime_error("write_lineage_origins: the last row of a leaf must be its root row");
    out << "LEAF:" << node_names.at(leaf_node[r0]) << "\t" << r1 - r0 + 1u << '\n';
    for (uint64_t w = 0; w < n_windows; ++w) {
      out << w * window;
      for (uint64_t r = r0; r <= r1; ++r) out << "\t" << origin[r * n_windows + w];
      out << "\t" << age[leaf * n_windows + w] << '\n';
    }
    r0 = r1 + 1u;
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

LineageOrigins read_lineage_origins(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad lineage-origins file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("lineage-origins file " + file + ": " + what); };
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
  LineageOrigins lo;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() != 6 || f[0] != "#samples" || f[2] != "window" || f[4] != "scale_exp") throw bad("bad header: " + line);
  lo.n_samples = std::stoull(f[1]);
  lo.window = std::stoull(f[3]);
  lo.scale_exp = std::stoi(f[5]);
  std::vector<std::vector<std::vector<uint64_t>>> leaves;   // [leaf][window][rows + 1]
  std::vector<uint64_t> leaf_rows;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    f = fields(line);
    if (f[0] == "#row") {
      if (f.size() != 4 || std::stoull(f[1]) != lo.row_leaf.size() || !leaves.empty()) throw bad("bad row line: " + line);
      lo.row_leaf.push_back(f[2]);
      lo.row_node.push_back(f[3]);
    } else if (line.compare(0, 5, "LEAF:") == 0) {
      if (f.size() != 2) throw bad("bad leaf line: " + line);
      leaf_rows.push_back(std::stoull(f[1]));
      leaves.emplace_back();
    } else {
      if (leaves.empty() || f.size() != leaf_rows.back() + 2u) throw bad("bad window line: " + line);
      if (std::stoull(f[0]) != leaves.back().size() * lo.window) throw bad("windows out of order: " + line);
      std::vector<uint64_t> v(f.size() - 1u);
      for (size_t i = 1; i < f.size(); ++i) v[i - 1u] = std::stoull(f[i]);
      leaves.back().push_back(v);
    }
  }
  const uint64_t R = lo.row_leaf.size(), L = leaves.size();
  uint64_t rows = 0;
  for (uint64_t n : leaf_rows) rows += n;
  if (rows != R) throw bad("the leaf blocks hold another number of rows than the row table");
  lo.n_windows = L ? leaves[0].size() : 0u;
  lo.origin.assign(R * lo.n_windows, 0u);
  lo.age.assign(L * lo.n_windows, 0u);
  uint64_t r0 = 0;
  for (uint64_t l = 0; l < L; ++l) {
    if (leaves[l].size() != lo.n_windows) throw bad("a leaf has another number of windows");
    for (uint64_t w = 0; w < lo.n_windows; ++w) {
      for (uint64_t i = 0; i < leaf_rows[l]; ++i) lo.origin[(r0 + i) * lo.n_windows + w] = leaves[l][w][i];
      lo.age[l * lo.n_windows + w] = leaves[l][w][leaf_rows[l]];
    }
    r0 += leaf_rows[l];
  }
  return lo;
}

void write_domain_stats(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_samples,
                        const uint64_t *hist, const uint64_t *len_sum) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  out << "#samples\t" << n_samples << "\tbins\t" << EPV_DOM_BINS << '\n';
  for (size_t v = 0; v < node_names.size(); ++v) {
    out << "NODE:" << node_names[v] << '\n';
    for (uint64_t st = 0; st < 2u; ++st) {
      const uint64_t *h = hist + (v * 2u + st) * EPV_DOM_BINS;
      uint64_t runs = 0;
      for (uint32_t b = 0; b < EPV_DOM_BINS; ++b) runs += h[b];
      out << "state\t" << st << "\truns\t" << runs << "\tsites\t" << len_sum[v * 2u + st] << '\n';
      for (uint32_t b = 0; b < EPV_DOM_BINS; ++b) {
        if (!h[b]) continue;
        uint64_t lo = 0, hi = 0;
        domain_bin_range(b, &lo, &hi);
        out << lo << "\t" << hi << "\t" << h[b] << '\n';
      }
    }
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

DomainStats read_domain_stats(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad domain-statistics file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("domain-statistics file " + file + ": " + what); };
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
  DomainStats ds;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() != 4 || f[0] != "#samples" || f[2] != "bins" || std::stoull(f[3]) != EPV_DOM_BINS)
    throw bad("bad header: " + line);
  ds.n_samples = std::stoull(f[1]);
  int state = -1;
  uint64_t runs = 0, seen = 0;
  auto end_state = [&] {
    if (state >= 0 && seen != runs) throw bad("the bins of a state do not add up to its runs");
  };
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    if (line.compare(0, 5, "NODE:") == 0) {
      end_state();
      if (state == 0 || (state < 0 && !ds.node_names.empty())) throw bad("a node without both states: " + line);
      ds.node_names.push_back(line.substr(5));
      ds.hist.resize(ds.node_names.size() * 2u * EPV_DOM_BINS, 0u);
      ds.len_sum.resize(ds.node_names.size() * 2u, 0u);
      state = -1;
      continue;
    }
    f = fields(line);
    if (ds.node_names.empty()) throw bad("a line before the first node: " + line);
    if (f[0] == "state") {
      end_state();
      if (f.size() != 6 || f[2] != "runs" || f[4] != "sites" || std::stoi(f[1]) != state + 1)
        throw bad("bad state line: " + line);
      state = std::stoi(f[1]);
      runs = std::stoull(f[3]);
      seen = 0;
      ds.len_sum[(ds.node_names.size() - 1u) * 2u + (size_t)state] = std::stoull(f[5]);
    } else {
      if (state < 0 || f.size() != 3) throw bad("bad bin line: " + line);
      const uint64_t lo = std::stoull(f[0]), hi = std::stoull(f[1]);
      const uint32_t b = epv_domain_bin(lo);
      uint64_t blo = 0, bhi = 0;
      domain_bin_range(b, &blo, &bhi);
      if (!lo || lo != blo || hi != bhi) throw bad("not the range of a bin: " + line);
      const uint64_t n = std::stoull(f[2]);
      ds.hist[((ds.node_names.size() - 1u) * 2u + (size_t)state) * EPV_DOM_BINS + b] += n;
      seen += n;
    }
  }
  end_state();
  if (state == 0 || (state < 0 && !ds.node_names.empty())) throw bad("the last node lacks a state");
  return ds;
}

void write_domain_turnover(const std::string &file, const std::vector<std::string> &branch_names, uint64_t n_samples,
                           const uint64_t *hist, const uint64_t *len_sum) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  out << "#samples\t" << n_samples << "\tbins\t" << EPV_DOM_BINS << '\n';
  for (size_t b = 0; b < branch_names.size(); ++b) {
    out << "BRANCH:" << branch_names[b] << '\n';
    for (uint64_t cls = 0; cls < 8u; ++cls) {   // (row, state, kept)
      const uint64_t *h = hist + (b * 8u + cls) * EPV_DOM_BINS;
      uint64_t runs = 0;
      for (uint32_t i = 0; i < EPV_DOM_BINS; ++i) runs += h[i];
      out << (cls & 4u ? "end" : "start") << "\tstate\t" << ((cls >> 1) & 1u) << "\tkept\t" << (cls & 1u) << "\truns\t"
          << runs << "\tsites\t" << len_sum[b * 8u + cls] << '\n';
      for (uint32_t i = 0; i < EPV_DOM_BINS; ++i) {
        if (!h[i]) continue;
        uint64_t lo = 0, hi = 0;
        domain_bin_range(i, &lo, &hi);
        out << lo << "\t" << hi << "\t" << h[i] << '\n';
      }
    }
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

DomainTurnover read_domain_turnover(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad domain-turnover file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("domain-turnover file " + file + ": " + what); };
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
  DomainTurnover dt;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() != 4 || f[0] != "#samples" || f[2] != "bins" || std::stoull(f[3]) != EPV_DOM_BINS)
    throw bad("bad header: " + line);
  dt.n_samples = std::stoull(f[1]);
  int cls = 7;   // the class of the last class line of the current branch (7: the branch is complete)
  uint64_t runs = 0, seen = 0;
  auto end_class = [&] {
    if (!dt.branch_names.empty() && cls >= 0 && seen != runs) throw bad("the bins of a class do not add up to its runs");
  };
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    if (line.compare(0, 7, "BRANCH:") == 0) {
      end_class();
      if (cls != 7) throw bad("a branch without all eight classes: " + line);
      dt.branch_names.push_back(line.substr(7));
      dt.hist.resize(dt.branch_names.size() * 8u * EPV_DOM_BINS, 0u);
      dt.len_sum.resize(dt.branch_names.size() * 8u, 0u);
      cls = -1;
      runs = seen = 0;
      continue;
    }
    f = fields(line);
    if (dt.branch_names.empty()) throw bad("a line before the first branch: " + line);
    if (f[0] == "start" || f[0] == "end") {
      end_class();
      if (f.size() != 9 || f[1] != "state" || f[3] != "kept" || f[5] != "runs" || f[7] != "sites")
        throw bad("bad class line: " + line);
      const int c = (f[0] == "end" ? 4 : 0) + 2 * std::stoi(f[2]) + std::stoi(f[4]);
      if (c != cls + 1 || (f[2] != "0" && f[2] != "1") || (f[4] != "0" && f[4] != "1")) throw bad("bad class line: " + line);
      cls = c;
      runs = std::stoull(f[6]);
      seen = 0;
      dt.len_sum[(dt.branch_names.size() - 1u) * 8u + (size_t)cls] = std::stoull(f[8]);
    } else {
      if (cls < 0 || f.size() != 3) throw bad("bad bin line: " + line);
      const uint64_t lo = std::stoull(f[0]), hi = std::stoull(f[1]);
      const uint32_t b = epv_domain_bin(lo);
      uint64_t blo = 0, bhi = 0;
      domain_bin_range(b, &blo, &bhi);
      if (!lo || lo != blo || hi != bhi) throw bad("not the range of a bin: " + line);
      const uint64_t n = std::stoull(f[2]);
      dt.hist[((dt.branch_names.size() - 1u) * 8u + (size_t)cls) * EPV_DOM_BINS + b] += n;
      seen += n;
    }
  }
  end_class();
  if (cls != 7) throw bad("the last branch lacks a class");
  return dt;
}

void write_spatial_correlation(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_samples,
                               uint64_t n_sites, uint32_t max_lag, const uint64_t *n11, const uint64_t *left1,
                               const uint64_t *right1) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  const size_t N = node_names.size(), R = N ? 2u * N - 1u : 0u, W = (size_t)max_lag + 1u;
  out << "#samples\t" << n_samples << "\tsites\t" << n_sites << "\tmax_lag\t" << max_lag << '\n';
  for (size_t r = 0; r < R; ++r) {
    if (r < N) out << "NODE:" << node_names[r] << '\n';
    else out << "BRANCH:" << node_names[r - N + 1u] << '\n';
    out << "ones\t" << n11[r * W] << '\n';
    for (size_t d = 1; d < W; ++d)
      out << d << '\t' << n11[r * W + d] << '\t' << left1[r * W + d] << '\t' << right1[r * W + d] << '\n';
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

SpatialCorrelation read_spatial_correlation(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad spatial-correlation file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("spatial-correlation file " + file + ": " + what); };
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
  SpatialCorrelation sc;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() != 6 || f[0] != "#samples" || f[2] != "sites" || f[4] != "max_lag") throw bad("bad header: " + line);
  sc.n_samples = std::stoull(f[1]);
  sc.n_sites = std::stoull(f[3]);
  const uint64_t L = std::stoull(f[5]);
  if (L == 0u || L > 1024u) throw bad("max_lag is 1 .. 1024: " + line);
  sc.max_lag = (uint32_t)L;
  const size_t W = (size_t)L + 1u;
  uint64_t next = W;   // the lag the next line of the current row holds (W: the row is complete)
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    if (line.compare(0, 5, "NODE:") == 0 || line.compare(0, 7, "BRANCH:") == 0) {
      if (next != W) throw bad("a row without all its lags before: " + line);
      sc.row_names.push_back(line);
      sc.n11.resize(sc.row_names.size() * W, 0u);
      sc.left1.resize(sc.row_names.size() * W, 0u);
      sc.right1.resize(sc.row_names.size() * W, 0u);
      next = 0;
      continue;
    }
    if (sc.row_names.empty()) throw bad("a line before the first row: " + line);
    f = fields(line);
    const size_t at = (sc.row_names.size() - 1u) * W + (size_t)next;
    if (next == 0u) {
      if (f.size() != 2 || f[0] != "ones") throw bad("bad ones line: " + line);
      sc.n11[at] = sc.left1[at] = sc.right1[at] = std::stoull(f[1]);
    } else {
      if (next >= W || f.size() != 4 || std::stoull(f[0]) != next) throw bad("bad lag line: " + line);
      sc.n11[at] = std::stoull(f[1]);
      sc.left1[at] = std::stoull(f[2]);
      sc.right1[at] = std::stoull(f[3]);
    }
    ++next;
  }
  if (next != W) throw bad("the last row lacks a lag");
  return sc;
}

// a 128-bit integer (low, high word) in decimal, and back
static std::string u128_str(uint64_t lo, uint64_t hi) {
  unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
  if (!v) return "0";
  std::string r;
  while (v) { r.push_back((char)('0' + (int)(v % 10u))); v /= 10u; }
  std::reverse(r.begin(), r.end());
  return r;
}
static void u128_parse(const std::string &t, uint64_t *lo, uint64_t *hi) {
  if (t.empty() || t.size() > 39) throw std::runtime_error("not a 128-bit integer: " + t);
  unsigned __int128 v = 0;
  for (char ch : t) {
    if (ch < '0' || ch > '9') throw std::runtime_error("not a 128-bit integer: " + t);
    v = v * 10u + (unsigned)(ch - '0');
  }
  *lo = (uint64_t)v;
  *hi = (uint64_t)(v >> 64);
}

void write_epoch_stats(const std::string &file, const std::vector<std::string> &node_names, int n_nodes, uint32_t P,
                       const double *branch_len, const int *scale_exp, const uint64_t *fixT, const uint64_t *closed,
                       uint64_t n_samples, const std::array<double, 8> &rates) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  char buf[64];
  auto g17 = [&](double v) { std::snprintf(buf, sizeof buf, "%.17g", v); return buf; };
  out << "#samples\t" << n_samples << "\tepochs\t" << P << '\n';
  for (int b = 1; b < n_nodes; ++b) {
    out << "NODE:" << node_names[b] << "\t" << g17(branch_len[b]) << "\t" << scale_exp[b] << '\n';
    const double inv = std::ldexp(1.0, -scale_exp[b]);
    for (uint32_t p = 0; p < P; ++p) {
      const uint64_t *o = closed + ((uint64_t)(b - 1) * P + p) * 24u;
      const uint64_t e = (uint64_t)((unsigned __int128)p * fixT[b] / P);
      out << g17(fixT[b] ? (double)e / (double)fixT[b] : 0.0);
      double J[8], D[8];
      for (int c = 0; c < 8; ++c) {
        out << "\t" << (int64_t)o[c];
        J[c] = (double)(int64_t)o[c];
      }
      for (int c = 0; c < 8; ++c) {
        out << "\t" << u128_str(o[8 + c], o[16 + c]);
        D[c] = (double)(((unsigned __int128)o[16 + c] << 64) | o[8 + c]) * inv;
      }
      out << "\t" << g17(regional_rate_factor(2, J, D, rates)) << '\n';   // (the sample count cancels)
    }
  }
  out.flush();
  if (!out) throw std::runtime_error("error writing: " + file);
}

EpochStats read_epoch_stats(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad epoch-statistics file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("epoch-statistics file " + file + ": " + what); };
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
  EpochStats es;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() != 4 || f[0] != "#samples" || f[2] != "epochs") throw bad("bad header: " + line);
  es.n_samples = std::stoull(f[1]);
  es.n_epochs = (uint32_t)std::stoul(f[3]);
  if (!es.n_epochs) throw bad("no epochs");
  uint32_t row = es.n_epochs;   // rows read of the current node
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    f = fields(line);
    if (line.compare(0, 5, "NODE:") == 0) {
      if (row != es.n_epochs) throw bad("node " + es.node_names.back() + " has another number of epochs");
      if (f.size() != 3) throw bad("bad node line: " + line);
      es.node_names.push_back(f[0].substr(5));
      es.branch_len.push_back(std::stod(f[1]));
      es.scale_exp.push_back(std::stoi(f[2]));
      es.closed.resize(es.node_names.size() * es.n_epochs * 24u, 0u);
      row = 0;
    } else {
      if (es.node_names.empty() || f.size() != 18 || row >= es.n_epochs) throw bad("bad epoch line: " + line);
      uint64_t *o = es.closed.data() + ((es.node_names.size() - 1u) * es.n_epochs + row) * 24u;
      es.start.push_back(std::stod(f[0]));
      for (int c = 0; c < 8; ++c) o[c] = (uint64_t)std::stoll(f[1 + c]);
      for (int c = 0; c < 8; ++c) u128_parse(f[9 + c], &o[8 + c], &o[16 + c]);
      es.factor.push_back(std::strtod(f[17].c_str(), nullptr));   // (takes "nan")
      ++row;
    }
  }
  if (row != es.n_epochs) throw bad("the last node has another number of epochs");
  return es;
}

}  // namespace epv

namespace epv {

void load_paths_and_tree(const std::string &paths_file, const std::string &tree_file, bool single_branch, bool verbose,
                         FlatPaths &paths, std::vector<std::string> &node_names, Tree &th) {
  if (verbose) std::cerr << "[READING PATHS FILE: " << paths_file << "]" << std::endl;
  std::vector<double> tot_times;
  paths = read_local_paths(paths_file, node_names, tot_times);

  if (single_branch) {
    if (verbose) std::cerr << "[INITIALIZING TWO NODE TREE WITH TIME: " << tot_times.back() << "]" << std::endl;
    th = Tree::single_branch(tot_times.back());
  } else {
    if (verbose) std::cerr << "[READING TREE: " << tree_file << "]" << std::endl;
    th = Tree::read(tree_file);
  }
  if (th.n_nodes() != paths.n_nodes)
    throw std::runtime_error("tree and paths file have different numbers of nodes");
  // The reference compares nothing here: branch lengths come from the tree, each Path keeps the
  // tot_time of the file, and scale_jump_times (ParamEstimation.cpp:369-380) brings the two
  // together at the end of the first iteration.  epievo_initialization without -b writes
  // rate-scaled tot_times next to an unscaled tree, so a mismatch is an ordinary input.  The
  // device keeps one length per branch, hence the same rescaling is applied at load time.
  for (int b = 1; b < th.n_nodes(); ++b)
    if (tot_times[b] != th.branches[b]) {
      if (!(tot_times[b] > 0.0) || !std::isfinite(tot_times[b]))
        throw std::runtime_error("paths of node " + th.node_names[b] + ": tot_time must be positive and finite");
      const double scale = th.branches[b] / tot_times[b];
      const uint64_t n = paths.n_sites;
      for (uint64_t k = paths.offsets[(uint64_t)(b - 1) * n]; k < paths.offsets[(uint64_t)b * n]; ++k)
        paths.jumps[k] *= scale;
      // always reported: first-iteration statistics of such an input differ from the reference's,
      // which keeps the file's tot_time until scale_jump_times ("tot_time")
      std::cerr << "[RESCALING PATHS OF NODE " << th.node_names[b] << ": tot_time " << tot_times[b]
           << " -> branch length " << th.branches[b] << "]" << std::endl;
    }
}

}  // namespace epv
