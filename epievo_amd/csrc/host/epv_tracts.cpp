// epv_tracts.cpp -- see epv_tracts.hpp
#include "epv_tracts.hpp"

#include <algorithm>
#include <fstream>
#include <stdexcept>

#include "epv_domains.hpp"

namespace epv {

namespace {
// a tract that is still open; left: the flank before it, unless it starts at the union's first site
struct Tract {
  uint64_t len = 0, gain = 0, loss = 0, left = 0;
  bool at_start = false;
};
struct Rec {
  uint64_t len, y, gain, loss, flank;
};
inline Rec unpack(uint64_t r) {
  return Rec{r & EPV_TRACT_LEN_MASK, (r >> EPV_TRACT_Y_SHIFT) & 1u, (r >> EPV_TRACT_GAIN_SHIFT) & 1u,
             (r >> EPV_TRACT_LOSS_SHIFT) & 1u, (r >> EPV_TRACT_FLANK_SHIFT) & 1u};
}
inline uint64_t pack(uint64_t len, uint64_t y, uint64_t gain, uint64_t loss, uint64_t flank) {
  return EPV_TRACT_SET | len | (y << EPV_TRACT_Y_SHIFT) | (gain << EPV_TRACT_GAIN_SHIFT) | (loss << EPV_TRACT_LOSS_SHIFT) |
         (flank << EPV_TRACT_FLANK_SHIFT);
}
inline void bin_tract(uint64_t *hist, uint64_t *len_sum, uint32_t b, uint64_t gain, uint64_t loss, uint64_t left,
                      uint64_t right, uint64_t len) {
  const uint64_t cls = (uint64_t)b * EPV_TRACT_CLASSES +
                       epv_tract_class(epv_tract_dir((uint32_t)gain, (uint32_t)loss), (uint32_t)left, (uint32_t)right);
  hist[cls * EPV_DOM_BINS + epv_domain_bin(len)] += 1u;
  len_sum[cls] += len;
}
}  // namespace

void tract_parts_merge(uint64_t n_parts, uint32_t B, uint64_t samples, const uint64_t *const *hists,
                       const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                       uint64_t *out_len_sum, uint64_t *out_edges) {
  const uint64_t nh = (uint64_t)B * EPV_TRACT_CLASSES * EPV_DOM_BINS, nl = (uint64_t)B * EPV_TRACT_CLASSES;
  std::fill(out_hist, out_hist + nh, 0u);
  std::fill(out_len_sum, out_len_sum + nl, 0u);
  for (uint64_t p = 0; p < n_parts; ++p) {
    for (uint64_t i = 0; i < nh; ++i) out_hist[i] += hists[p][i];
    for (uint64_t i = 0; i < nl; ++i) out_len_sum[i] += len_sums[p][i];
  }
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t b = 0; b < B; ++b) {
      const uint64_t at = (s * B + b) * 2u;
      bool any = false, open = false, first_set = false;
      Tract cur;
      uint64_t first = 0, y_first = 0, y_last = 0;
      // the open tract meets an unchanged site of state `right`: the union's first record, or a tract to bin
      auto close = [&](uint64_t right) {
        if (cur.at_start) { first = pack(cur.len, y_first, cur.gain, cur.loss, right); first_set = true; }
        else bin_tract(out_hist, out_len_sum, b, cur.gain, cur.loss, cur.left, right, cur.len);
        open = false;
      };
      // the tract a piece continues, or the one it begins after the site before it
      auto extend = [&](const Rec &r) {
        if (!open) { cur = Tract{}; cur.left = y_last; cur.at_start = !any; open = true; }
        cur.len += r.len; cur.gain |= r.gain; cur.loss |= r.loss;
      };
      for (uint64_t p = 0; p < n_parts; ++p) {
        const uint64_t f = edges[p][at], l = edges[p][at + 1u];
        if (!f && !l) continue;   // a part of no sites
        const Rec fr = unpack(f), lr = unpack(l);
        if (!any) y_first = fr.y;
        if (f & EPV_TRACT_WHOLE) {
          extend(fr);
        } else {
          if (fr.len) { extend(fr); close(fr.flank); }
          else if (open) close(fr.y);
          if (lr.len) { cur = Tract{lr.len, lr.gain, lr.loss, lr.flank, false}; open = true; }
        }
        y_last = lr.y;
        any = true;
      }
      if (!any) { out_edges[at] = out_edges[at + 1u] = 0u; continue; }
      if (open && cur.at_start) {
        out_edges[at] = pack(cur.len, y_first, cur.gain, cur.loss, 0u) | EPV_TRACT_WHOLE;
        out_edges[at + 1u] = pack(cur.len, y_last, cur.gain, cur.loss, 0u) | EPV_TRACT_WHOLE;
        continue;
      }
      out_edges[at] = first_set ? first : pack(0u, y_first, 0u, 0u, 0u);
      out_edges[at + 1u] = open ? pack(cur.len, y_last, cur.gain, cur.loss, cur.left) : pack(0u, y_last, 0u, 0u, 0u);
    }
}

void tract_part_close(uint32_t B, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges) {
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t b = 0; b < B; ++b) {
      const uint64_t f = edges[(s * B + b) * 2u], l = edges[(s * B + b) * 2u + 1u];
      if (!f && !l) continue;
      const Rec fr = unpack(f), lr = unpack(l);
      if (f & EPV_TRACT_WHOLE) {
        bin_tract(hist, len_sum, b, fr.gain, fr.loss, EPV_TRACT_NONE, EPV_TRACT_NONE, fr.len);
        continue;
      }
      if (fr.len) bin_tract(hist, len_sum, b, fr.gain, fr.loss, EPV_TRACT_NONE, fr.flank, fr.len);
      if (lr.len) bin_tract(hist, len_sum, b, lr.gain, lr.loss, lr.flank, EPV_TRACT_NONE, lr.len);
    }
}

namespace {
const char *const kDirName[EPV_TRACT_DIRS] = {"gain", "loss", "mixed"};
const char *const kFlankName[3] = {"0", "1", "-"};
}  // namespace

void write_change_tracts(const std::string &file, const std::vector<std::string> &branch_names, uint64_t n_samples,
                         const uint64_t *hist, const uint64_t *len_sum) {
  std::ofstream out(file);
  if (!out) throw std::runtime_error("bad output file: " + file);
  out << "#samples\t" << n_samples << "\tbins\t" << EPV_DOM_BINS << '\n';
  for (size_t b = 0; b < branch_names.size(); ++b) {
    out << "BRANCH:" << branch_names[b] << '\n';
    for (uint32_t cls = 0; cls < EPV_TRACT_CLASSES; ++cls) {
      const uint64_t *h = hist + (b * EPV_TRACT_CLASSES + cls) * EPV_DOM_BINS;
      uint64_t tracts = 0;
      for (uint32_t i = 0; i < EPV_DOM_BINS; ++i) tracts += h[i];
      if (!tracts) continue;
      out << kDirName[cls / 9u] << "\tleft\t" << kFlankName[(cls / 3u) % 3u] << "\tright\t" << kFlankName[cls % 3u]
          << "\ttracts\t" << tracts << "\tsites\t" << len_sum[b * EPV_TRACT_CLASSES + cls] << '\n';
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

ChangeTracts read_change_tracts(const std::string &file) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("bad change-tract file: " + file);
  auto bad = [&](const std::string &what) { return std::runtime_error("change-tract file " + file + ": " + what); };
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
  auto index_of = [](const std::string &s, const char *const *names, int n) {
    for (int i = 0; i < n; ++i) if (s == names[i]) return i;
    return -1;
  };
  ChangeTracts ct;
  std::string line;
  if (!std::getline(in, line)) throw bad("empty");
  std::vector<std::string> f = fields(line);
  if (f.size() != 4 || f[0] != "#samples" || f[2] != "bins" || std::stoull(f[3]) != EPV_DOM_BINS)
    throw bad("bad header: " + line);
  ct.n_samples = std::stoull(f[1]);
  int cls = -1;   // the class of the last class line of the current branch
  uint64_t tracts = 0, seen = 0;
  auto end_class = [&] {
    if (cls >= 0 && seen != tracts) throw bad("the bins of a class do not add up to its tracts");
  };
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    if (line.compare(0, 7, "BRANCH:") == 0) {
      end_class();
      ct.branch_names.push_back(line.substr(7));
      ct.hist.resize(ct.branch_names.size() * EPV_TRACT_CLASSES * EPV_DOM_BINS, 0u);
      ct.len_sum.resize(ct.branch_names.size() * EPV_TRACT_CLASSES, 0u);
      cls = -1;
      tracts = seen = 0;
      continue;
    }
    f = fields(line);
    if (ct.branch_names.empty()) throw bad("a line before the first branch: " + line);
    const size_t b = ct.branch_names.size() - 1u;
    const int dir = index_of(f[0], kDirName, (int)EPV_TRACT_DIRS);
    if (dir >= 0) {
      end_class();
      if (f.size() != 9 || f[1] != "left" || f[3] != "right" || f[5] != "tracts" || f[7] != "sites")
        throw bad("bad class line: " + line);
      const int left = index_of(f[2], kFlankName, 3), right = index_of(f[4], kFlankName, 3);
      const int c = dir * 9 + left * 3 + right;
      if (left < 0 || right < 0 || c <= cls) throw bad("bad class line: " + line);
      cls = c;
      tracts = std::stoull(f[6]);
      if (!tracts) throw bad("a class without tracts: " + line);
      seen = 0;
      ct.len_sum[b * EPV_TRACT_CLASSES + (size_t)cls] = std::stoull(f[8]);
    } else {
      if (cls < 0 || f.size() != 3) throw bad("bad bin line: " + line);
      const uint64_t lo = std::stoull(f[0]), hi = std::stoull(f[1]);
      const uint32_t bin = epv_domain_bin(lo);
      uint64_t blo = 0, bhi = 0;
      domain_bin_range(bin, &blo, &bhi);
      if (!lo || lo != blo || hi != bhi) throw bad("not the range of a bin: " + line);
      const uint64_t n = std::stoull(f[2]);
      ct.hist[(b * EPV_TRACT_CLASSES + (size_t)cls) * EPV_DOM_BINS + bin] += n;
      seen += n;
    }
  }
  end_class();
  return ct;
}

}  // namespace epv
