// average_paths -- drop-in for the reference's program of the same name
// (src/prog/average_paths.cpp): the average history of many sampled local_paths files, per node,
// site and point of an equally spaced time grid, in the reference's output format.
// Differences: the files are read in sorted name order (the reference takes the order of the
// directory listing; only the branch lengths printed, the first file's, depend on it), and every
// node averages its own paths (the reference reads node 1's for points >= 1 of every node,
// average_paths.cpp:39).  epievo_est_histories -a writes the same format from the
// counts kept on the GPU during the sampling, without the files.
#include <dirent.h>

#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <stdexcept>

#include "epv_io.hpp"
#include "epv_options.hpp"

using std::cerr;
using std::endl;
using std::string;
using std::vector;

static string strip_path(const string &full) {
  const size_t p = full.find_last_of('/');
  return p == string::npos ? full : full.substr(p + 1);
}

static vector<string> local_paths_files(const string &dir) {
  DIR *d = ::opendir(dir.c_str());
  if (!d) throw std::runtime_error("cannot read directory: " + dir);
  vector<string> files;
  static const string suffix = "local_paths";
  while (const dirent *e = ::readdir(d)) {
    const string name = e->d_name;
    if (name.size() >= suffix.size() && name.compare(name.size() - suffix.size(), suffix.size(), suffix) == 0)
      files.push_back(dir + "/" + name);
  }
  ::closedir(d);
  std::sort(files.begin(), files.end());
  return files;
}

int main(int argc, const char **argv) {
  try {
    bool VERBOSE = false;
    string outfile;
    size_t n_points = 100;
    epv::OptionParser opt_parse(strip_path(argv[0]), "average local paths", "<input directory>");
    opt_parse.add_opt("outfile", 'o', "output file", true, outfile);
    opt_parse.add_opt("npoints", 'n', "number of bins", false, n_points);
    opt_parse.add_opt("verbose", 'v', "print more run info", false, VERBOSE);
    vector<string> leftover_args;
    opt_parse.parse(argc, argv, leftover_args);
    if (argc == 1 || opt_parse.help_requested()) {
      cerr << opt_parse.help_message() << endl << opt_parse.about_message() << endl;
      return EXIT_SUCCESS;
    }
    if (opt_parse.option_missing()) {
      cerr << opt_parse.option_missing_message() << endl;
      return EXIT_SUCCESS;
    }
    if (leftover_args.size() < 1) {
      cerr << opt_parse.option_missing_message() << endl;
      return EXIT_SUCCESS;
    }
    if (n_points < 2 || n_points > 0xffffffffu)
      throw std::runtime_error("-n: the number of points must be at least 2");
    const string paths_dir(leftover_args[0]);
    if (VERBOSE) cerr << "[READING PATHS FROM: " << paths_dir << "]" << endl;
    const vector<string> files = local_paths_files(paths_dir);
    if (files.empty()) throw std::runtime_error("no *local_paths files in " + paths_dir);

    vector<string> names0;
    vector<double> branch_len;
    vector<uint32_t> counts;
    uint64_t n_sites = 0;
    int n_nodes = 0;
    for (size_t f = 0; f < files.size(); ++f) {
      vector<string> names;
      vector<double> tot_times;
      const epv::FlatPaths p = epv::read_local_paths(files[f], names, tot_times);
      if (p.n_nodes < 2) throw std::runtime_error(files[f] + ": no paths");
      if (f == 0) {
        names0 = names;
        branch_len = tot_times;
        n_sites = p.n_sites;
        n_nodes = p.n_nodes;
      } else if (p.n_nodes != n_nodes) {
        throw std::runtime_error(files[f] + ": " + std::to_string(p.n_nodes) + " nodes, " + files[0] + " has " +
                                 std::to_string(n_nodes));
      } else if (p.n_sites != n_sites) {
        throw std::runtime_error(files[f] + ": " + std::to_string(p.n_sites) + " sites, " + files[0] + " has " +
                                 std::to_string(n_sites));
      } else if (names != names0) {
        throw std::runtime_error(files[f] + ": node names differ from those of " + files[0]);
      }
      if (VERBOSE) cerr << "[ADDING: " << files[f] << "]" << endl;
      epv::add_path_counts(p, tot_times.data(), (uint32_t)n_points, counts);
    }
    if (VERBOSE) cerr << "[WRITING OUTPUT TO: " << outfile << "]" << endl;
    epv::write_path_average(outfile, names0, n_nodes, n_sites, (uint32_t)n_points, branch_len.data(), counts.data(),
                            files.size());
  } catch (const std::exception &e) {
    cerr << e.what() << endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
