// epv_io.hpp -- the text formats that form the drop-in surface of the hot path
// (SURVEY.md section 8b "file formats to keep"): Newick tree, local_paths, states.
#ifndef EPV_IO_HPP
#define EPV_IO_HPP

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "epv_sim.hpp"  // FlatPaths

namespace epv {

// Tree in the pre-order array form the sampler consumes -- the fields of the
// reference's TreeHelper (src/libepievo/TreeHelper.hpp:47-51).
struct Tree {
  std::vector<uint32_t> subtree_sizes;
  std::vector<uint32_t> parent_ids;
  std::vector<double> branches;
  std::vector<std::string> node_names;
  std::vector<bool> name_generated;   // node_<k> made up for an unnamed node: not printed back
  int n_nodes() const { return (int)subtree_sizes.size(); }
  bool is_leaf(int node) const { return subtree_sizes[node] == 1; }

  // operator>>(istream&, PhyloTree&) + TreeHelper(PhyloTreePreorder)
  // (src/libepievo/PhyloTree.cpp:110-122,144-203,286-301; TreeHelper.cpp:43-51)
  static Tree parse(const std::string &newick);
  static Tree read(const std::string &tree_file);
  // the two-node tree of TreeHelper(const double &evo_time), TreeHelper.cpp:53-60
  static Tree single_branch(double evo_time);
  // PhyloTree::Newick_format (PhyloTree.cpp:110-122) with the current branch lengths
  std::string newick() const;
};

// read_paths(path_file, node_names, paths) (src/libepievo/Path.cpp:123-148), returned
// node-major.  tot_times[b] is the tot_time column of node b (taken from its first
// site; every site of a node must agree, else std::runtime_error).
FlatPaths read_local_paths(const std::string &path_file, std::vector<std::string> &node_names,
                           std::vector<double> &tot_times);

// the writers of src/prog/epievo_est_params_histories.cpp:56-75 (root line, then per
// node "NODE:<name>" and "site\tinit\ttot_time\tjump\t..." at max_digits10)
void write_local_paths(const std::string &path_file, const std::vector<std::string> &node_names,
                       int n_nodes, uint64_t n_sites, const double *tot_times,
                       const uint8_t *init, const uint64_t *offsets, const double *jumps);

// average_paths (src/prog/average_paths.cpp:31-45), one sample: for every node b >= 1, site s
// and point i of the grid t_0 = 0, t_1 = bin, t_{i+1} = t_i + bin (bin = tot_times[b] / (P - 1)),
// counts[((b-1) * n_sites + s) * P + i] += the path's init state at i = 0, state_at_time(t_i)
// (Path.cpp:106-111) at i >= 1.  The reference reads node 1's path for i >= 1 of every node
// (average_paths.cpp:39); this reads node b's own.
void add_path_counts(const FlatPaths &paths, const double *tot_times, uint32_t n_points,
                     std::vector<uint32_t> &counts);
// write_output of average_paths.cpp:49-63: "NODE:<root>", then per node "NODE:<name>\t<branch_len>"
// and one line of P tab-separated averages counts / n_samples per site, default ostream formatting
void write_path_average(const std::string &file, const std::vector<std::string> &node_names, int n_nodes,
                        uint64_t n_sites, uint32_t n_points, const double *branch_len, const uint32_t *counts,
                        uint64_t n_samples);

// the window sums of the branch-event planes (epv_get_branch_event_windows), integers only so that files
// compare exactly: "#samples\t<S>\twindow\t<W>", then per non-root node in pre-order
// "NODE:<name>\t<branch_len>" (default ostream formatting) and one line per window: the window's first
// global site and sums[(p * (n_nodes-1) + b-1) * n_windows + w] for the six planes p, tab-separated
void write_branch_events(const std::string &file, const std::vector<std::string> &node_names, int n_nodes,
                         uint64_t n_windows, uint64_t window, const double *branch_len, const uint64_t *sums,
                         uint64_t n_samples);

// the chain mixing diagnostics per window of `window` sites (the file host.read_mixing of the Python package reads):
// "#epievo-mixing 1", the lines "samples S", "moved_pairs M", "max_lag K", "pairs p_1 .. p_K", "window W",
// "first_window 0", a comment line, then per window: its index, its sites, the integer sum of moved, and as
// floating point (%.17g, nan where undefined) the move rate moved / (M sites), the pooled rho_k = sum_p cov_k(p) /
// sum_p var(p) for k = 1 .. K and tau of it (Geyer's initial positive sequence).  words[K + 2] = S, M, p_1 .. p_K;
// moved[site]; sums[r * n_sites + site], rows S1, S2, C_1 .. C_K
void write_mixing(const std::string &file, uint32_t max_lag, const uint64_t *words, uint64_t n_sites, uint64_t window,
                  const uint32_t *moved, const uint64_t *sums);

// the window sums of the change-pattern rows (epv_get_change_pattern_windows), integers only:
// "#samples\t<S>\twindow\t<W>\tsites\t<n>", a line "#rows" with the name of every row (jumps_1 .. jumps_6,
// jumps_7plus, one_branch, parallel_gain, parallel_loss, gain_and_loss, reverted_only, sole_gain:<node> and
// sole_loss:<node> per non-root node, clade_changed:<node> per internal non-root node, from subtree_sizes), then one
// line per window: the window's first global site and sums[r * n_windows + w] for the rows r, tab-separated
void write_change_patterns(const std::string &file, const std::vector<std::string> &node_names,
                           const std::vector<uint32_t> &subtree_sizes, uint32_t n_rows, uint64_t n_sites,
                           uint64_t n_windows, uint64_t window, const uint64_t *sums, uint64_t n_samples);

// the regional sufficient statistics of epievo_est_histories -r (epv_get_window_stats):
//   "#samples\t<S>\twindow\t<W>", then per non-root node in pre-order "NODE:<name>\t<branch length>\t<k_b>"
//   (%.17g; D integers are in units of 2^-k_b) and one line per window: its first global site, J[0..7] and
//   D[0..7] as the integer sums over the samples, tab-separated; after the last node one block "NODE:all"
//   with a line per window: first global site, sum_b J[8] (integers), sum_b D[8] per sample in time units
//   (%.17g) and the regional rate factor under `rates` (epv::regional_rate_factor; "nan" for an empty window).
// counts: [w][b-1][16] int64; J, D: [w][b-1][8] per sample (epv_window_counts_to_stats); scale_exp: k_b per
// node, index 0 = root (epv_window_stats_scale_exps: the accumulator's own).
struct WindowStats {
  uint64_t n_samples = 0, window = 0, n_windows = 0;
  std::vector<std::string> node_names;   // non-root nodes
  std::vector<double> branch_len;        // per non-root node
  std::vector<int> scale_exp;            // k_b per non-root node
  std::vector<int64_t> counts;           // [w][b][16]
  std::vector<int64_t> all_J;            // [w][8]
  std::vector<double> all_D;             // [w][8]
  std::vector<double> factor;            // [w]
};
void write_window_stats(const std::string &file, const std::vector<std::string> &node_names, int n_nodes,
                        uint64_t n_windows, uint64_t window, const double *branch_len, const int *scale_exp,
                        const int64_t *counts, uint64_t n_samples, const double *J, const double *D,
                        const std::array<double, 8> &rates);
WindowStats read_window_stats(const std::string &file);

// the lineage origin maps of epievo_est_histories -O (epv_get_lineage_origin_windows), integers only:
//   "#samples\t<S>\twindow\t<W>\tscale_exp\t<k>" (an age integer is a time in units of 2^-k), then the row
//   table, one line "#row\t<r>\t<leaf name>\t<node name>" per row (the node whose branch the row belongs to;
//   a leaf's last row, the root row, names the root), then per leaf in node order "LEAF:<name>\t<rows>" and
//   one line per window: its first global site, the window sums of the leaf's origin rows from the leaf's own
//   branch up to the root row, and the window's age sum, tab-separated.
// origin: [r][w], age: [l][w] (uint64); leaf_node, branch_node: per row (epv_lineage_origin_rows)
struct LineageOrigins {
  uint64_t n_samples = 0, window = 0, n_windows = 0;
  int scale_exp = 0;
  std::vector<std::string> row_leaf, row_node;   // names per row
  std::vector<uint64_t> origin;                  // [r][w]
  std::vector<uint64_t> age;                     // [l][w]
};
void write_lineage_origins(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_rows,
                           const uint32_t *leaf_node, const uint32_t *branch_node, uint64_t n_windows, uint64_t window,
                           int scale_exp, const uint64_t *origin, const uint64_t *age, uint64_t n_samples);
LineageOrigins read_lineage_origins(const std::string &file);

// the domain size spectra of epievo_est_histories -d (the closed result of epv_get_domain_stats), integers only:
//   "#samples\t<S>\tbins\t128", then per node "NODE:<name>", per state a line
//   "state\t<0|1>\truns\t<count>\tsites\t<len_sum>" and one line "lo\thi\tcount" per nonzero bin (lo .. hi: the run
//   lengths of the bin).  Readers divide by the samples.  hist: [v][state][bin], len_sum: [v][state] (uint64)
struct DomainStats {
  uint64_t n_samples = 0;
  std::vector<std::string> node_names;
  std::vector<uint64_t> hist;      // [v][2][128]
  std::vector<uint64_t> len_sum;   // [v][2]
};
void write_domain_stats(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_samples,
                        const uint64_t *hist, const uint64_t *len_sum);
DomainStats read_domain_stats(const std::string &file);

// the domain turnover of epievo_est_histories -R (the closed result of epv_get_domain_turnover), integers only:
//   "#samples\t<S>\tbins\t128", then per branch "BRANCH:<child node name>", per row (start, end), state and kept
//   a line "<start|end>\tstate\t<0|1>\tkept\t<0|1>\truns\t<count>\tsites\t<len_sum>" and one line "lo\thi\tcount"
//   per nonzero bin.  hist: [2 b + row][state][kept][bin], len_sum: [2 b + row][state][kept] (uint64)
struct DomainTurnover {
  uint64_t n_samples = 0;
  std::vector<std::string> branch_names;
  std::vector<uint64_t> hist;      // [2 B][2][2][128]
  std::vector<uint64_t> len_sum;   // [2 B][2][2]
};
void write_domain_turnover(const std::string &file, const std::vector<std::string> &branch_names, uint64_t n_samples,
                           const uint64_t *hist, const uint64_t *len_sum);
DomainTurnover read_domain_turnover(const std::string &file);

// the spatial correlations of epievo_est_histories -C (the closed result of epv_get_spatial_correlation), integers
// only: "#samples\t<S>\tsites\t<n>\tmax_lag\t<L>", then per row "NODE:<name>" (the N nodes) or "BRANCH:<child node
//   name>" (the B branches), a line "ones\t<n11[0]>" and one line "d\tn11\tleft1\tright1" per lag 1 .. L.
//   n11, left1, right1: [N + B][L + 1] (uint64)
struct SpatialCorrelation {
  uint64_t n_samples = 0, n_sites = 0;
  uint32_t max_lag = 0;
  std::vector<std::string> row_names;   // "NODE:<name>" or "BRANCH:<name>"
  std::vector<uint64_t> n11, left1, right1;   // [R][L + 1]
};
void write_spatial_correlation(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_samples,
                               uint64_t n_sites, uint32_t max_lag, const uint64_t *n11, const uint64_t *left1,
                               const uint64_t *right1);
SpatialCorrelation read_spatial_correlation(const std::string &file);

// the epoch statistics of epievo_est_histories -E (epv_get_epoch_stats closed by epv::epoch_close):
//   "#samples\t<S>\tepochs\t<P>", then per non-root node in pre-order "NODE:<name>\t<branch length>\t<k_b>"
//   (%.17g; D integers are in units of 2^-k_b) and one line per epoch: the epoch's start as a fraction of
//   the branch (E_p / fixT_b, %.17g), J[0..7] and D[0..7] as the integer sums over the samples (D up to 128
//   bits, in decimal) and the epoch's rate factor under `rates` (epv::regional_rate_factor of the one
//   branch and epoch; "nan" without dwell time), tab-separated.
// closed: [b-1][p][24] as epv::epoch_close writes it; scale_exp, fixT, branch_len: per node, index 0 = root.
struct EpochStats {
  uint64_t n_samples = 0;
  uint32_t n_epochs = 0;
  std::vector<std::string> node_names;   // non-root nodes
  std::vector<double> branch_len;        // per non-root node
  std::vector<int> scale_exp;            // k_b per non-root node
  std::vector<uint64_t> closed;          // [b][p][24]: J[8], D low words [8], D high words [8]
  std::vector<double> start;             // [b][p]
  std::vector<double> factor;            // [b][p]
};
void write_epoch_stats(const std::string &file, const std::vector<std::string> &node_names, int n_nodes, uint32_t P,
                       const double *branch_len, const int *scale_exp, const uint64_t *fixT, const uint64_t *closed,
                       uint64_t n_samples, const std::array<double, 8> &rates);
EpochStats read_epoch_stats(const std::string &file);

// the inputs of the E-step programs (epievo_est_params_histories.cpp:166-200): the local_paths file,
// then the Newick tree or, with single_branch, the two-node tree of the file's last tot_time.  The
// device keeps one length per branch, so paths whose tot_time differs from the tree's branch length
// are rescaled to it here (reported on stderr; INTEGRATION.md, "tot_time")
void load_paths_and_tree(const std::string &paths_file, const std::string &tree_file, bool single_branch, bool verbose,
                         FlatPaths &paths, std::vector<std::string> &node_names, Tree &th);

// read_states_file (src/libepievo/epievo_utils.cpp:90-125): states[seq][site]
void read_states_file(const std::string &states_file, std::vector<std::string> &names,
                      std::vector<std::vector<uint8_t>> &states);
// the same file with missing data: `N` or `n` marks a missing cell (missing[seq][site] = 1, its state 0);
// every other character keeps read_states_file's meaning
void read_states_file_missing(const std::string &states_file, std::vector<std::string> &names,
                              std::vector<std::vector<uint8_t>> &states, std::vector<std::vector<uint8_t>> &missing);
// -m/--missing of the E-step programs: the leaf cells a states file marks missing, as the whole-genome mask
// of SingleSiteSampler::set_unobserved over `paths` ([(b-1) * n_sites + site]).  Columns are matched to the
// leaves by name (every leaf needs one; columns of internal nodes are ignored) and the file needs one row per
// site.  Throws, naming leaf and site, where an observed cell differs from the paths' leaf end state.
std::vector<uint8_t> unobserved_leaf_cells(const std::string &states_file, const Tree &th, const FlatPaths &paths,
                                           uint64_t &n_unobserved, uint64_t &n_leaf_cells);
// The regions file of a genome (-G; the chrom.sizes shape): one line per region, `name <whitespace> n_sites`, in
// the order of the paths file; a line that starts with # is a comment, an empty line is skipped.  Every region
// holds at least 3 sites and the lengths sum to n_sites.  -> the lengths (SingleSiteSampler::set_regions).  A
// violation throws naming the line
std::vector<uint64_t> read_regions(const std::string &regions_file, uint64_t n_sites);
// a file of the same shape whose tokens are probabilities of state 1: a real number in [0, 1], or `N`/`n` for
// no information (0.5).  probs[seq][site]; any other token is stored as +infinity
void read_leaf_probs_file(const std::string &probs_file, std::vector<std::string> &names,
                          std::vector<std::vector<float>> &probs);
// -l/--leaf-probs of the E-step programs: the whole-genome table of SingleSiteSampler::set_leaf_evidence over
// `paths` ([(b-1) * n_sites + site], NaN = none).  Columns and rows are matched as unobserved_leaf_cells does.
// A token that is exactly 0 or 1 as a float32 is data: it gets no entry (the cell stays pinned) and must agree
// with the paths' leaf end state.  Throws, naming leaf and site, where it does not, or where a token of a leaf
// column is not a probability.  n_evidence counts the entries set.
std::vector<float> leaf_evidence_cells(const std::string &probs_file, const Tree &th, const FlatPaths &paths,
                                       uint64_t &n_evidence, uint64_t &n_leaf_cells);

}  // namespace epv

#endif
