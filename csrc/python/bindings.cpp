// Python bindings (pybind11) for the native engine: `locust_amd._locust`.
//
// The hot path stays in C++/HIP; Python only moves the input bytes in and formatted
// results out.  The GPU engine is created lazily, so importing the module never touches
// the HIP runtime (the driver's CPU-only build check imports it on a machine without GPU).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <optional>
#include <string>
#include <tuple>

#include "locust/devcache.hpp"
#include "locust/device/radix_sched.hpp"
#include "locust/dict_stage.hpp"
#include "locust/dist.hpp"
#include "locust/dstring.hpp"
#include "locust/device/regex.hpp"
#include "locust/engine.hpp"
#include "locust/exch_stage.hpp"
#include "locust/gen.hpp"
#include "locust/io.hpp"
#include "locust/stage.hpp"
#include "locust/numa.hpp"
#include "locust/partmap.hpp"
#include "locust/shm.hpp"

namespace py = pybind11;
using namespace locust;

namespace {

struct PyResult {
  WordCountResult r;
  py::list entries() const {
    py::list out;
    EntryVals vals(r);
    for (const auto& e : r.entries)
      out.append(py::make_tuple(py::bytes(key_to_string(e.key)), vals.next(e), e.count));
    return out;
  }
  py::dict times() const {
    py::dict d;
    d["h2d_ms"] = r.times.h2d_ms;
    d["map_ms"] = r.times.map_ms;
    d["process_ms"] = r.times.process_ms;
    d["reduce_ms"] = r.times.reduce_ms;
    d["d2h_ms"] = r.times.d2h_ms;
    d["wall_ms"] = r.times.wall_ms;
    d["gpu_ms"] = r.times.gpu_ms;
    d["host_launch_ms"] = r.times.host_launch_ms;
    d["host_wait_ms"] = r.times.host_wait_ms;
    d["host_copy_ms"] = r.times.host_copy_ms;
    d["ref_map_ms"] = r.times.ref_map_ms;
    d["ref_process_ms"] = r.times.ref_process_ms;
    d["ref_reduce_ms"] = r.times.ref_reduce_ms;
    d["graph"] = r.times.graph;
    d["lean"] = r.times.lean;
    return d;
  }
  py::bytes format(bool cpu_format) const {
    std::string s;
    (cpu_format ? format_cpu_output : format_gpu_output)(r, &s);
    return py::bytes(s);
  }
};

// A top-K result: the rank-ordered (key, val, count) entries and the job's statistics.
struct PyTopResult {
  TopResult t;
  py::list entries() const {
    py::list out;
    for (const auto& e : t.entries)
      out.append(py::make_tuple(py::bytes(key_to_string(e.key)), e.val, e.count));
    return out;
  }
  py::dict times() const {
    py::dict d = PyResult{WordCountResult{}}.times();
    d["h2d_ms"] = t.times.h2d_ms;
    d["map_ms"] = t.times.map_ms;
    d["process_ms"] = t.times.process_ms;
    d["reduce_ms"] = t.times.reduce_ms;
    d["d2h_ms"] = t.times.d2h_ms;
    d["wall_ms"] = t.times.wall_ms;
    d["gpu_ms"] = t.times.gpu_ms;
    d["select_ms"] = t.select_ms;
    return d;
  }
  py::bytes format(bool cpu_format) const {
    std::string s;
    format_top_output(t, cpu_format, &s);
    return py::bytes(s);
  }
};

// engine.hpp "corpus": a segment table as [(id, first_line, base, lines)]
std::vector<std::tuple<u32, u64, u64, u64>> segment_rows(const IndexSegments& t) {
  std::vector<std::tuple<u32, u64, u64, u64>> out;
  for (size_t i = 0; i < t.segs.size(); ++i)
    out.emplace_back(t.segs[i].id, t.segs[i].first_line, t.segs[i].base, t.lines_of(i));
  return out;
}

// An inverted index: the word job's entries and the CSR postings behind them.
struct PySearchResult;
struct PyIndexResult {
  IndexResult x;
  JobConfig cfg;  // the job's delimiters and max_key_len: what search() validates terms by
  PySearchResult search(const std::vector<std::vector<std::string>>& queries,
                        const std::vector<int>& any, const py::object& rank, bool wildcard,
                        const std::vector<u64>& within,
                        const std::vector<std::vector<std::string>>& exclude, bool glob,
                        bool ignore_case, const py::object& show, bool fuzzy, bool regex,
                        const py::object& tally,
                        const std::vector<std::vector<u32>>& files, u32 by_file) const;
  py::list entries() const { return PyResult{x.words}.entries(); }
  py::list postings() const {
    py::list out;
    for (const u32 l : x.postings) out.append(l);
    return out;
  }
  // the postings as little-endian u32 words (np.frombuffer(..., dtype="<u4"))
  py::bytes postings_bytes() const {
    return py::bytes(reinterpret_cast<const char*>(x.postings.data()),
                     x.postings.size() * sizeof(u32));
  }
  // The lines of `key` (one per occurrence; unique: each line once); empty if absent.
  py::list lines(const std::string& key, bool unique) const {
    py::list out;
    if (key.size() > (size_t)kKeyBytes) return out;
    PackedKey k;
    pack_key(key.data(), (int)key.size(), k.w);
    EntryVals vals(x.words);
    for (const auto& e : x.words.entries) {
      const u64 val = vals.next(e);
      const int c = key_compare(e.key.w, k.w);
      if (c < 0) continue;
      if (c == 0)
        for (u64 j = val; j < val + e.count && j < x.postings.size(); ++j)
          if (!unique || j == val || x.postings[j] != x.postings[j - 1]) out.append(x.postings[j]);
      break;
    }
    return out;
  }
  py::dict times() const {
    py::dict d = PyResult{x.words}.times();
    d["index_ms"] = x.index_ms;
    return d;
  }
  py::bytes format() const {
    std::string s;
    format_index_output(x, &s);
    return py::bytes(s);
  }
};

// A search result: per query the ascending global line numbers, and the terms' counts
// (ranked: the best lines first, and their scores).
struct PySearchResult {
  SearchResult r;
  void check(size_t i) const {
    if (i >= r.queries.size()) throw py::index_error("query index out of range");
  }
  py::list lines(size_t i) const {
    check(i);
    py::list out;
    for (u64 j = r.offsets[i]; j < r.offsets[i + 1]; ++j) out.append(r.lines[j]);
    return out;
  }
  py::list hits() const {
    py::list out;
    for (size_t i = 0; i + 1 < r.offsets.size(); ++i) out.append(r.offsets[i + 1] - r.offsets[i]);
    return out;
  }
  py::list scores(size_t i) const {
    check(i);
    py::list out;
    if (r.rank_k)
      for (u64 j = r.offsets[i]; j < r.offsets[i + 1]; ++j) out.append(r.scores[j]);
    return out;
  }
  py::list matches() const {
    py::list out;
    for (const u64 m : r.matches) out.append(m);
    return out;
  }
  py::list term_counts(size_t i) const {
    check(i);
    py::list out;
    for (size_t t = 0; t < r.queries[i].terms.size(); ++t)
      out.append(r.term_counts[i * kSearchMaxTerms + t]);
    return out;
  }
  py::dict times() const {
    py::dict d = PyResult{WordCountResult{}}.times();
    d["h2d_ms"] = r.times.h2d_ms;
    d["map_ms"] = r.times.map_ms;
    d["process_ms"] = r.times.process_ms;
    d["reduce_ms"] = r.times.reduce_ms;
    d["d2h_ms"] = r.times.d2h_ms;
    d["wall_ms"] = r.times.wall_ms;
    d["gpu_ms"] = r.times.gpu_ms;
    d["index_ms"] = r.index_ms;
    d["search_ms"] = r.search_ms;
    d["show_ms"] = r.show_ms;
    d["tally_ms"] = r.tally_ms;
    return d;
  }
  py::bytes format(bool mark) const {
    std::string s;
    format_search_output(r, &s, mark);
    return py::bytes(s);
  }
  // show: query i's entries -- the shown bytes of each, and each one's (start, len, mask) spans
  py::list text(size_t i) const {
    check(i);
    py::list out;
    if (r.show_bytes)
      for (u64 j = r.offsets[i]; j < r.offsets[i + 1]; ++j)
        out.append(py::bytes(r.text.data() + r.text_off[j], r.text_off[j + 1] - r.text_off[j]));
    return out;
  }
  // tally: query i's words, [(key bytes, count)], count descending, key ascending
  py::list tally(size_t i) const {
    check(i);
    py::list out;
    if (r.tally_k)
      for (u64 j = r.tally_off[i]; j < r.tally_off[i + 1]; ++j)
        out.append(py::make_tuple(py::bytes(key_to_string(r.tally_keys[j])), r.tally_counts[j]));
    return out;
  }
  // by file: query i's returned lines' file ids / file-local numbers (parallel to lines(i))
  py::list files(size_t i) const {
    check(i);
    py::list out;
    if (r.by_file == kByFile)
      for (u64 j = r.offsets[i]; j < r.offsets[i + 1]; ++j) out.append(r.line_file[j]);
    return out;
  }
  py::list local_lines(size_t i) const {
    check(i);
    py::list out;
    if (r.by_file == kByFile)
      for (u64 j = r.offsets[i]; j < r.offsets[i + 1]; ++j) out.append(r.line_local[j]);
    return out;
  }
  // by file: [(id, count)] over the files with a returned line of query i, ids ascending
  py::list file_hits(size_t i) const {
    check(i);
    py::list out;
    if (r.by_file)
      for (u64 f = r.file_off[i]; f < r.file_off[i + 1]; ++f)
        out.append(py::make_tuple(r.file_ids[f], r.file_counts[f]));
    return out;
  }
  py::list tally_words() const {
    py::list out;
    for (const u64 w : r.tally_words) out.append(w);
    return out;
  }
  py::list tally_tokens() const {
    py::list out;
    for (const u64 w : r.tally_tokens) out.append(w);
    return out;
  }
  py::list text_off() const {
    py::list out;
    for (const u64 o : r.text_off) out.append(o);
    return out;
  }
  py::list span_off() const {
    py::list out;
    for (const u64 o : r.span_off) out.append(o);
    return out;
  }
  py::list spans(size_t i) const {
    check(i);
    py::list out;
    if (r.show_bytes)
      for (u64 j = r.offsets[i]; j < r.offsets[i + 1]; ++j) {
        py::list one;
        for (u64 k = r.span_off[j]; k < r.span_off[j + 1]; ++k)
          one.append(py::make_tuple(r.spans[3 * k], r.spans[3 * k + 1], r.spans[3 * k + 2]));
        out.append(one);
      }
    return out;
  }
};

// queries: term lists; any[i]: query i's mode -- 0 `all`, 2 `phrase`, 3 `near`, every other
// value `any` (any.size() == queries.size()).  wildcard: make_search_query's rule for a
// trailing `*`.  within: empty, or one window per query (0: none; check_search_queries holds
// it against the mode).  exclude: empty, or one list of exclusion terms per query (an empty
// list: none).  glob: make_search_query's rule for `*` and `?` anywhere in a term; fuzzy: its
// rule for a trailing `~1` or `~2`.  any[i] == 4: an `expr` query -- queries[i] holds one
// element, the expression (make_search_expr; cfg: the job's delimiters); a window or exclusion
// terms given for it are refused by the engines' check_search_queries.
std::vector<SearchQuery> to_queries(const JobConfig& cfg,
                                    const std::vector<std::vector<std::string>>& queries,
                                    const std::vector<int>& any, bool wildcard,
                                    const std::vector<u64>& within,
                                    const std::vector<std::vector<std::string>>& exclude,
                                    bool glob, bool fuzzy = false, bool regex = false,
                                    const std::vector<std::vector<u32>>& files = {}) {
  LOCUST_CHECK_ARG(any.size() == queries.size(), "search: one mode per query");
  LOCUST_CHECK_ARG(files.empty() || files.size() == queries.size(),
                   "search: one file set (files) per query, or none");
  LOCUST_CHECK_ARG(within.empty() || within.size() == queries.size(),
                   "search: one window (within) per query, or none");
  LOCUST_CHECK_ARG(exclude.empty() || exclude.size() == queries.size(),
                   "search: one list of exclusion terms (exclude) per query, or none");
  std::vector<SearchQuery> out(queries.size());
  for (size_t i = 0; i < queries.size(); ++i) {
    if (any[i] == 4) {
      LOCUST_CHECK_ARG(queries[i].size() == 1,
                       "search: an expr query is one expression (bytes, or a one-element list), "
                       "not " + std::to_string(queries[i].size()) + " terms");
      out[i] = make_search_expr(queries[i][0], cfg, wildcard, glob, fuzzy, regex);
      // (a window or exclusion terms on it: carried along as given, for check_search_queries,
      // which every engine runs before anything else, to refuse)
      if (!within.empty()) out[i].within = within[i];
      if (!exclude.empty() && !exclude[i].empty()) {
        out[i].terms.insert(out[i].terms.end(), exclude[i].begin(), exclude[i].end());
        out[i].excluded = (u32)exclude[i].size();
      }
      continue;
    }
    out[i] = make_search_query(queries[i],
                               any[i] == 0   ? SearchMode::kAll
                               : any[i] == 2 ? SearchMode::kPhrase
                               : any[i] == 3 ? SearchMode::kNear
                                             : SearchMode::kAny,
                               wildcard, within.empty() ? 0 : within[i],
                               exclude.empty() ? std::vector<std::string>() : exclude[i], glob,
                               fuzzy, regex);
  }
  // "file sets": segment ids, as given (check_search_queries refuses a set that is not ascending)
  for (size_t i = 0; i < files.size(); ++i) out[i].files = files[i];
  return out;
}

// rank: None (the unranked answer) or K >= 1 -> the engines' rank_k (0: unranked).
u64 to_rank(const py::object& rank) {
  if (rank.is_none()) return 0;
  long long k = 0;
  try {
    k = rank.cast<long long>();
  } catch (const py::cast_error&) {  // (not an integer, or one past 64 bits)
  }
  LOCUST_CHECK_ARG(k >= 1 && k < (1ll << 32),
                   "search: rank takes None or 1 <= K < 2^32, not " +
                       py::str(rank).cast<std::string>());
  return (u64)k;
}

// show: None or 0 (no show), or N -> the engines' show.
u64 to_show(const py::object& show) {
  if (show.is_none()) return 0;
  long long n = -1;
  try {
    n = show.cast<long long>();
  } catch (const py::cast_error&) {  // (not an integer, or one past 64 bits)
  }
  LOCUST_CHECK_ARG(n >= 0 && n <= (long long)kShowMaxBytes,
                   "search: show takes None or 1 <= N <= " + std::to_string(kShowMaxBytes) +
                       ", not " + py::str(show).cast<std::string>());
  return (u64)n;
}

// tally: None or 0 (no tally), or K -> the engines' tally.
u64 to_tally(const py::object& tally) {
  if (tally.is_none()) return 0;
  long long n = -1;
  try {
    n = tally.cast<long long>();
  } catch (const py::cast_error&) {  // (not an integer, or one past 64 bits)
  }
  LOCUST_CHECK_ARG(n >= 0 && n <= (long long)kTopKMax,
                   "search: tally takes None or 1 <= K <= kTopKMax = " + std::to_string(kTopKMax) +
                       ", not " + py::str(tally).cast<std::string>());
  return (u64)n;
}

PySearchResult PyIndexResult::search(const std::vector<std::vector<std::string>>& queries,
                                     const std::vector<int>& any, const py::object& rank,
                                     bool wildcard, const std::vector<u64>& within,
                                     const std::vector<std::vector<std::string>>& exclude, bool glob,
                        bool ignore_case, const py::object& show, bool fuzzy, bool regex,
                        const py::object& tally,
                        const std::vector<std::vector<u32>>& files, u32 by_file) const {
  const std::vector<SearchQuery> q =
      to_queries(cfg, queries, any, wildcard, within, exclude, glob, fuzzy, regex, files);
  const u64 k = to_rank(rank);
  const u64 n = to_show(show);
  const u64 tk = to_tally(tally);
  py::gil_scoped_release nogil;
  return PySearchResult{search_index(x, q, cfg, k, ignore_case, n, tk, by_file)};
}

TextInput as_input(const std::string& text, u64 first_line = 0) {
  TextInput in;
  in.data = text.data();
  in.bytes = text.size();
  in.num_lines = count_lines(text.data(), text.size());
  in.first_line = first_line;
  return in;
}

PackedKey to_key(const std::string& s) {
  PackedKey k;
  pack_key(s.data(), (int)std::min<size_t>(s.size(), kKeyBytes), k.w);
  return k;
}

class PyGpuEngine {
 public:
  py::dict stats() const {
    const GpuWordCount::Stats st = eng_.stats();
    py::dict d;
    d["retunes"] = st.retunes;
    d["fallbacks"] = st.fallbacks;
    d["planned_passes"] = st.planned_passes;
    d["process_path"] = std::string(st.process_path);
    d["devplan_failed"] = st.devplan_failed;
    d["device_bytes"] = st.device_bytes;
    d["hbm_free"] = st.hbm_free;
    d["hbm_total"] = st.hbm_total;
    d["streaming"] = st.streaming;
    d["chunk_bytes"] = st.chunk_bytes;
    d["map_window"] = st.map_window;
    d["search_bytes"] = st.search_bytes;
    d["index_store_bytes"] = st.index_store_bytes;
    return d;
  }
  PyGpuEngine(const JobConfig& cfg, u64 max_bytes, u64 max_lines)
      : eng_(cfg, max_bytes, max_lines), max_bytes_(max_bytes) {}
  GpuWordCount& engine() { return eng_; }
  PyResult run(const std::string& text) {
    py::gil_scoped_release nogil;
    return PyResult{eng_.run(as_input(text))};
  }
  std::vector<py::bytes> map_stage(const std::string& text) {
    std::vector<PackedKey> toks;
    {
      py::gil_scoped_release nogil;
      toks = eng_.run_map_stage(as_input(text), nullptr);
    }
    std::vector<py::bytes> out;
    for (const auto& k : toks) out.emplace_back(key_to_string(k));
    return out;
  }
  PyResult reduce_stage(const std::vector<std::string>& keys) {
    std::vector<PackedKey> toks;
    for (const auto& s : keys) toks.push_back(to_key(s));
    py::gil_scoped_release nogil;
    return PyResult{eng_.run_reduce_stage(toks.data(), toks.size())};
  }
  // counts: None, or one u64 per key; then the sorted counts are a third element.
  py::tuple sort_keys(const std::vector<std::string>& keys,
                      const std::optional<std::vector<u64>>& counts) {
    LOCUST_CHECK_ARG(!counts || counts->size() == keys.size(), "sort_keys: one count per key");
    std::vector<PackedKey> toks;
    for (const auto& s : keys) toks.push_back(to_key(s));
    std::vector<PackedKey> sorted;
    std::vector<u32> perm;
    std::vector<u64> sorted_counts;
    {
      py::gil_scoped_release nogil;
      // (an empty vector's data() may be null, which would read as "no counts")
      static const u64 none = 0;
      const u64* c = !counts ? nullptr : counts->empty() ? &none : counts->data();
      perm = eng_.sort_keys(toks.data(), toks.size(), &sorted, c, &sorted_counts);
    }
    std::vector<py::bytes> out;
    for (const auto& k : sorted) out.emplace_back(key_to_string(k));
    if (counts) return py::make_tuple(out, perm, sorted_counts);
    return py::make_tuple(out, perm);
  }
  std::vector<py::bytes> compact_slots(const std::vector<u32>& line_counts,
                                       const std::vector<std::string>& slot_keys) {
    std::vector<PackedKey> slots;
    for (const auto& s : slot_keys) slots.push_back(to_key(s));
    LOCUST_CHECK_ARG(slots.size() == line_counts.size() * (u64)eng_.config().emits_per_line,
                     "need num_lines * emits_per_line slot keys");
    std::vector<PackedKey> dense;
    {
      py::gil_scoped_release nogil;
      dense = eng_.compact_slots(line_counts.data(), (u32)line_counts.size(), slots.data());
    }
    std::vector<py::bytes> out;
    for (const auto& k : dense) out.emplace_back(key_to_string(k));
    return out;
  }
  PyResult reduce_sorted(const std::vector<std::string>& keys) {
    std::vector<PackedKey> toks;
    for (const auto& s : keys) toks.push_back(to_key(s));
    py::gil_scoped_release nogil;
    return PyResult{eng_.reduce_sorted(toks.data(), toks.size())};
  }
  // runs: lists of (key bytes, count), each sorted with distinct keys.
  PyResult merge_runs(const std::vector<std::vector<std::pair<std::string, u64>>>& runs) {
    std::vector<std::vector<KeyCount>> rr(runs.size());
    for (size_t q = 0; q < runs.size(); ++q)
      for (const auto& kc : runs[q]) {
        KeyCount rec;
        const PackedKey k = to_key(kc.first);
        for (int w = 0; w < kKeyWords; ++w) rec.w[w] = k.w[w];
        rec.count = kc.second;
        rr[q].push_back(rec);
      }
    py::gil_scoped_release nogil;
    return PyResult{eng_.merge_runs(rr)};
  }
  // Top-K jobs: the selection runs on the device, only the winners cross PCIe.
  PyTopResult run_top(const std::string& text, u32 k) {
    py::gil_scoped_release nogil;
    return PyTopResult{eng_.run_top(as_input(text), k)};
  }
  PyTopResult run_top_text(const HostText& t, u32 k) {
    py::gil_scoped_release nogil;
    return PyTopResult{eng_.run_top(t.input(), k)};
  }
  PyTopResult run_top_file(const std::string& path, u32 k) {
    py::gil_scoped_release nogil;
    auto src = open_file_source(path);
    return PyTopResult{eng_.run_top_source(*src, k)};
  }
  // The word job and the inverted index behind it, on the device.
  PyIndexResult run_index(const std::string& text, u64 first_line) {
    py::gil_scoped_release nogil;
    return PyIndexResult{eng_.run_index(as_input(text, first_line)), eng_.config()};
  }
  PyIndexResult run_index_text(const HostText& t, u64 first_line) {
    py::gil_scoped_release nogil;
    return PyIndexResult{eng_.run_index(t.input(first_line)), eng_.config()};
  }
  // The word job, the index and a batch of all/any queries answered on the device.
  PySearchResult run_search(const std::string& text,
                            const std::vector<std::vector<std::string>>& queries,
                            const std::vector<int>& any, u64 first_line,
                            const py::object& rank, bool wildcard,
                            const std::vector<u64>& within,
                            const std::vector<std::vector<std::string>>& exclude, bool glob,
                        bool ignore_case, const py::object& show, bool fuzzy, bool regex,
                        const py::object& tally,
                        const std::vector<std::vector<u32>>& files, u32 by_file) {
    const std::vector<SearchQuery> q =
        to_queries(eng_.config(), queries, any, wildcard, within, exclude, glob, fuzzy, regex, files);
    const u64 k = to_rank(rank);
    const u64 n = to_show(show);
    const u64 tk = to_tally(tally);
    py::gil_scoped_release nogil;
    return PySearchResult{eng_.run_search(as_input(text, first_line), q, k, ignore_case, n, tk, by_file)};
  }
  PySearchResult run_search_text(const HostText& t,
                                 const std::vector<std::vector<std::string>>& queries,
                                 const std::vector<int>& any, u64 first_line,
                                 const py::object& rank, bool wildcard,
                            const std::vector<u64>& within,
                            const std::vector<std::vector<std::string>>& exclude, bool glob,
                        bool ignore_case, const py::object& show, bool fuzzy, bool regex,
                        const py::object& tally,
                        const std::vector<std::vector<u32>>& files, u32 by_file) {
    const std::vector<SearchQuery> q =
        to_queries(eng_.config(), queries, any, wildcard, within, exclude, glob, fuzzy, regex, files);
    const u64 k = to_rank(rank);
    const u64 n = to_show(show);
    const u64 tk = to_tally(tally);
    py::gil_scoped_release nogil;
    return PySearchResult{eng_.run_search(t.input(first_line), q, k, ignore_case, n, tk, by_file)};
  }
  PySearchResult search_resident(const std::vector<std::vector<std::string>>& queries,
                                 const std::vector<int>& any, const py::object& rank,
                                 bool wildcard, const std::vector<u64>& within,
                                 const std::vector<std::vector<std::string>>& exclude, bool glob,
                        bool ignore_case, const py::object& show, bool fuzzy, bool regex,
                        const py::object& tally,
                        const std::vector<std::vector<u32>>& files, u32 by_file) {
    const std::vector<SearchQuery> q =
        to_queries(eng_.config(), queries, any, wildcard, within, exclude, glob, fuzzy, regex, files);
    const u64 k = to_rank(rank);
    const u64 n = to_show(show);
    const u64 tk = to_tally(tally);
    py::gil_scoped_release nogil;
    return PySearchResult{eng_.search_resident(q, k, ignore_case, n, tk, by_file)};
  }
  // One more block of whole lines into the resident index, merged on the device.
  IndexAppend append_index(const std::string& text, u64 first_line, bool new_file) {
    py::gil_scoped_release nogil;
    return eng_.append_index(as_input(text, first_line), new_file);
  }
  // "corpus": the resident segments, [(id, first_line, base, lines)]
  std::vector<std::tuple<u32, u64, u64, u64>> segments() { return segment_rows(eng_.segments()); }
  // The oldest `lines` lines out of the resident index, compacted on the device.
  IndexDrop drop_index(u64 lines) {
    py::gil_scoped_release nogil;
    return eng_.drop_index(lines);
  }
  // The resident index downloaded, whatever it was built from.
  PyIndexResult index_resident() {
    py::gil_scoped_release nogil;
    return PyIndexResult{eng_.index_resident(), eng_.config()};
  }
  // records: (key bytes, count), sorted by key with distinct keys -- the kernels alone.
  PyTopResult top_counts(const std::vector<std::pair<std::string, u64>>& records, u32 k) {
    std::vector<KeyCount> recs;
    recs.reserve(records.size());
    for (const auto& kc : records) {
      KeyCount rec;
      const PackedKey key = to_key(kc.first);
      for (int w = 0; w < kKeyWords; ++w) rec.w[w] = key.w[w];
      rec.count = kc.second;
      recs.push_back(rec);
    }
    py::gil_scoped_release nogil;
    return PyTopResult{eng_.top_counts(recs.data(), recs.size(), k)};
  }
  u64 capacity() const { return eng_.token_capacity(); }
  // Stage the text in the engine's pinned buffer once; run_loaded() then skips the copy.
  void load(const std::string& text) {
    loaded_in_ = as_input(text);
    if (text.size() <= eng_.text_capacity()) {
      std::memcpy(eng_.input_buffer(), text.data(), text.size());
      loaded_ = eng_.input_buffer();
    } else {
      // larger than one device pass: keep it pinned, the engine streams it in chunks
      big_ = std::make_unique<HostText>(text.size());
      std::memcpy(big_->data(), text.data(), text.size());
      big_->set_size(text.size(), loaded_in_.num_lines);
      loaded_ = big_->data();
    }
    loaded_in_.data = loaded_;
  }
  PyResult run_loaded() {
    LOCUST_CHECK_ARG(loaded_ != nullptr, "call load() first");
    py::gil_scoped_release nogil;
    return PyResult{eng_.run(loaded_in_)};
  }
  // Text in pinned host memory, any size (larger than the capacity: streamed in chunks).
  PyResult run_text(const HostText& t) {
    py::gil_scoped_release nogil;
    return PyResult{eng_.run(t.input())};
  }
  // A file streamed through a streaming engine (the CLI's run_direct past one pass).
  PyResult run_file(const std::string& path) {
    py::gil_scoped_release nogil;
    auto src = open_file_source(path);
    return PyResult{eng_.run_source(*src)};
  }

 private:
  GpuWordCount eng_;
  u64 max_bytes_;
  std::unique_ptr<HostText> big_;
  char* loaded_ = nullptr;
  TextInput loaded_in_;
};

py::list strtok_r_tokens(const std::string& line, const std::string& delims) {
  std::string buf = line;
  py::list out;
  char* save = nullptr;
  for (char* t = d_strtok_r(&buf[0], delims.c_str(), &save); t;
       t = d_strtok_r(nullptr, delims.c_str(), &save))
    out.append(py::bytes(t));
  return out;
}

LocalComm local_comm(const std::string& c) {
  if (c == "auto") return LocalComm::kAuto;
  if (c == "loopback") return LocalComm::kLoopback;
  if (c == "rccl") return LocalComm::kRccl;
  throw Error("comm must be auto, loopback or rccl, not " + c);
}

PyResult run_multi(const std::string& text, const DistConfig& cfg, const std::string& comm) {
  TextInput in = as_input(text);
  const LocalComm lc = local_comm(comm);
  py::gil_scoped_release nogil;
  DistResult d = run_single_process_multi_gpu(cfg, in, lc);
  return PyResult{d.result};
}

py::dict dist_to_dict(const DistResult& d);

py::list run_multi_schedule(const std::string& text, const std::vector<DistConfig>& schedule,
                            const std::string& comm) {
  TextInput in = as_input(text);
  const LocalComm lc = local_comm(comm);
  std::vector<DistResult> rs;
  {
    py::gil_scoped_release nogil;
    rs = run_single_process_schedule(schedule, in, lc);
  }
  py::list out;
  for (const auto& d : rs) out.append(py::make_tuple(PyResult{d.result}, dist_to_dict(d)));
  return out;
}

py::dict dist_to_dict(const DistResult& d) {
  py::dict x;
  x["map_ms"] = d.map_ms;
  x["shuffle_ms"] = d.shuffle_ms;
  x["device_exchange"] = d.device_exchange;
  x["host_syncs"] = d.host_syncs;
  x["output_bytes"] = d.output_bytes;
  x["reduce_ms"] = d.reduce_ms;
  x["gather_ms"] = d.gather_ms;
  x["total_ms"] = d.total_ms;
  x["local_records"] = d.local_records;
  x["sent_bytes"] = d.sent_bytes;
  x["recv_bytes"] = d.recv_bytes;
  x["range_tokens"] = d.range_tokens;
  x["range_unique"] = d.range_unique;
  x["strategy"] = d.strategy == DistStrategy::kGather  ? "gather"
                  : d.strategy == DistStrategy::kLocal ? "local"
                                                       : "shuffle";
  x["input_bytes"] = d.input_bytes;
  x["input_streamed"] = d.input_streamed;
  x["peer_p2p"] = d.peer_p2p;
  x["rccl_clique"] = d.rccl_clique;
  x["pinned_bytes"] = d.pinned_bytes;
  x["shared_pinned_bytes"] = d.shared_pinned_bytes;
  x["hbm_device_bytes"] = d.hbm_device_bytes;
  x["hbm_free_bytes"] = d.hbm_free_bytes;
  x["hbm_total_bytes"] = d.hbm_total_bytes;
  x["hbm_used_bytes"] = d.hbm_used_bytes;
  x["sent_to"] = d.sent_to;
  x["recv_from"] = d.recv_from;
  return x;
}

// A file's multi-rank job in this process: every rank reads only its own byte range.
py::tuple run_multi_file(const std::string& path, const DistConfig& cfg, const std::string& comm) {
  const LocalComm lc = local_comm(comm);
  std::vector<DistResult> ranks;
  DistResult d;
  {
    py::gil_scoped_release nogil;
    d = run_single_process_file(cfg, path, lc, &ranks);
  }
  py::list infos;
  for (const auto& x : ranks) infos.append(dist_to_dict(x));
  return py::make_tuple(PyResult{d.result}, infos);
}

// A rank of a multi-process job: its communicator and engine live across runs.
class PyDistRank {
 public:
  PyDistRank(const DistConfig& cfg, int rank, const std::string& comm, const std::string& host,
             int port, u64 max_bytes, u64 max_lines, double timeout_s, int listen_fd)
      : cfg_(cfg), max_bytes_(max_bytes) {
    py::gil_scoped_release nogil;
    if (comm == "tcp") {
      comm_ = make_tcp_comm(rank, cfg.world, host, port, timeout_s, listen_fd);
    } else if (comm == "tcpdev") {
      comm_ = make_staged_device_comm(make_tcp_comm(rank, cfg.world, host, port, timeout_s, listen_fd));
    } else if (comm == "rccl") {
      comm_ = make_rccl_comm(rank, cfg.world, cfg.job.device, host, port, timeout_s, listen_fd);
    } else {
      throw Error("unknown communicator " + comm);
    }
    engines_.push_back(make_engine(max_bytes, max_lines));
    eng_ = engines_[0].get();
  }
  // Another engine on the same communicator (a second input shape, e.g. the synthetic
  // strong-scaling config next to the Hamlet headline); returns its index for use_engine.
  // Every rank must add and select engines in the same order.
  int add_engine(u64 max_bytes, u64 max_lines) {
    py::gil_scoped_release nogil;
    engines_.push_back(make_engine(max_bytes, max_lines));
    return (int)engines_.size() - 1;
  }
  void use_engine(int i) {
    LOCUST_CHECK_ARG(i >= 0 && (size_t)i < engines_.size(), "no such engine");
    eng_ = engines_[(size_t)i].get();
    engine_caps_idx_ = i;
    loaded_ = false;  // load() the new engine's shard
  }
  py::tuple run(const std::string& shard_text_bytes, u64 first_line) {
    TextInput in = as_input(shard_text_bytes, first_line);
    DistResult d;
    {
      py::gil_scoped_release nogil;
      d = run_distributed(cfg_, *comm_, *eng_, in);
    }
    return py::make_tuple(PyResult{d.result}, dist_to_dict(d));
  }
  // Keep the shard resident (in the engine's pinned buffer when it has one) so repeated
  // runs skip the Python->native copy, like GpuEngine.load().
  void load(const std::string& shard_text_bytes, u64 first_line) {
    loaded_in_ = as_input(shard_text_bytes, first_line);
    char* pinned = eng_->input_buffer();
    if (pinned) {
      LOCUST_CHECK_ARG(shard_text_bytes.size() <= caps_[(size_t)engine_caps_idx_],
                       "shard exceeds engine capacity");
      if (shard_text_bytes.size() <= cfg_.job.chunk_bytes || !cfg_.job.chunk_bytes) {
        std::memcpy(pinned, shard_text_bytes.data(), shard_text_bytes.size());
        loaded_in_.data = pinned;
      } else {
        big_ = std::make_unique<HostText>(shard_text_bytes.size());
        std::memcpy(big_->data(), shard_text_bytes.data(), shard_text_bytes.size());
        loaded_in_.data = big_->data();
      }
    } else {
      loaded_text_ = shard_text_bytes;
      loaded_in_.data = loaded_text_.data();
    }
    loaded_ = true;
  }
  // A HostText shard (pinned; may exceed the engine capacity: streamed).  The caller
  // keeps it alive (the binding ties its lifetime to this rank).
  void load_text(const HostText& t, u64 first_line) {
    loaded_in_ = t.input(first_line);
    loaded_ = true;
  }
  py::tuple run_loaded() {
    LOCUST_CHECK_ARG(loaded_, "call load() first");
    DistResult d;
    {
      py::gil_scoped_release nogil;
      d = run_distributed(cfg_, *comm_, *eng_, loaded_in_);
    }
    return py::make_tuple(PyResult{d.result}, dist_to_dict(d));
  }
  void barrier() {
    py::gil_scoped_release nogil;
    comm_->barrier();
  }
  // Max over ranks of a double (timing aggregation for the benchmark).
  double allreduce_max(double v) {
    std::vector<double> all((size_t)comm_->size());
    {
      py::gil_scoped_release nogil;
      comm_->allgather_host(&v, all.data(), sizeof(double));
    }
    double m = v;
    for (double x : all) m = std::max(m, x);
    return m;
  }
  // Every rank's bytes (any length) on every rank: lengths first, then padded payloads.
  py::list allgather_bytes(const std::string& mine) {
    const u64 P = (u64)comm_->size();
    std::vector<u64> lens(P);
    std::vector<char> all;
    u64 mx = 0;
    {
      py::gil_scoped_release nogil;
      const u64 n = mine.size();
      comm_->allgather_host(&n, lens.data(), sizeof(u64));
      for (u64 l : lens) mx = std::max(mx, l);
      std::string pad = mine;
      pad.resize(std::max<u64>(mx, 1));
      all.resize(std::max<u64>(mx, 1) * P);
      comm_->allgather_host(pad.data(), all.data(), std::max<u64>(mx, 1));
    }
    py::list out;
    for (u64 r = 0; r < P; ++r)
      out.append(py::bytes(all.data() + r * std::max<u64>(mx, 1), lens[r]));
    return out;
  }
  int rank() const { return comm_->rank(); }
  int size() const { return comm_->size(); }
  int comm_count() const { return comm_->comm_count(); }
  std::string comm_name() const { return comm_->name(); }
  void set_strategy(DistStrategy s) { cfg_.strategy = s; }

 private:
  std::unique_ptr<ShardEngine> make_engine(u64 max_bytes, u64 max_lines) {
    caps_.push_back(max_bytes);
    return cfg_.job.backend == Backend::kGpu ? make_gpu_shard_engine(cfg_.job, max_bytes, max_lines)
                                             : make_cpu_shard_engine(cfg_.job);
  }
  DistConfig cfg_;
  u64 max_bytes_;
  std::unique_ptr<Communicator> comm_;
  std::vector<std::unique_ptr<ShardEngine>> engines_;
  std::vector<u64> caps_;
  int engine_caps_idx_ = 0;
  ShardEngine* eng_ = nullptr;
  bool loaded_ = false;
  std::unique_ptr<HostText> big_;
  std::string loaded_text_;
  TextInput loaded_in_;
};

// ---- stage entry points of the device shuffle (locust/exch_stage.hpp) ----
// Keys cross as blobs of 32-byte packed keys: each key its bytes, NUL padded -- the
// big-endian form of its four words, so bytes compare like the packed keys do.
std::vector<PackedKey> keys_from_blob(const std::string& b) {
  LOCUST_CHECK_ARG(b.size() % kKeyBytes == 0, "a key blob holds 32 bytes per key");
  std::vector<PackedKey> out(b.size() / kKeyBytes);
  for (size_t i = 0; i < out.size(); ++i) pack_key(b.data() + i * kKeyBytes, kKeyBytes, out[i].w);
  return out;
}
template <class Rec>  // PackedKey or KeyCount
py::bytes blob_from_keys(const Rec* k, size_t n) {
  std::string b(n * kKeyBytes, '\0');
  for (size_t i = 0; i < n; ++i)
    for (int j = 0; j < kKeyBytes; ++j)
      b[i * kKeyBytes + j] = (char)(k[i].w[j >> 3] >> (56 - 8 * (j & 7)));
  return py::bytes(b);
}
std::vector<KeyCount> records_from(const std::string& keys, const std::vector<u64>& counts) {
  const std::vector<PackedKey> k = keys_from_blob(keys);
  LOCUST_CHECK_ARG(k.size() == counts.size(), "one count per key");
  std::vector<KeyCount> r(k.size());
  for (size_t i = 0; i < k.size(); ++i) {
    for (int w = 0; w < kKeyWords; ++w) r[i].w[w] = k[i].w[w];
    r[i].count = counts[i];
  }
  return r;
}
py::dict exch_plan_dict(const ExchStagePlan& p, u32 P) {
  py::dict d;
  d["off"] = std::vector<u64>(p.ctl.off, p.ctl.off + P + 1);
  d["flags"] = p.ctl.flags;
  d["max_bucket"] = p.ctl.max_bucket;
  py::list slots;
  for (const ExchStageSlot& s : p.slots) {
    py::dict e;
    e["status"] = s.header.status;
    e["record_flags"] = s.header.record_flags;
    e["n"] = s.header.n;
    e["slot_cap"] = s.header.slot_cap;
    // the header's other fields (map statistics of the gather strategy, padding)
    e["rest"] = std::vector<u64>{s.header.lines, s.header.tokens, s.header.overflow_lines,
                                 s.header.truncated, s.header.max_key_len, s.header.pad[0],
                                 s.header.pad[1]};
    e["keys"] = blob_from_keys(s.records.data(), s.records.size());
    std::vector<u64> counts(s.records.size());
    for (size_t i = 0; i < counts.size(); ++i) counts[i] = s.records[i].count;
    e["counts"] = counts;
    e["dirty_records"] = s.dirty_records;
    e["tail_intact"] = s.tail_intact;
    slots.append(e);
  }
  d["slots"] = slots;
  return d;
}

// A slot of the shuffle tail's stage entry points: (80 header bytes, key blob, counts).
using PyMergeSlot = std::tuple<std::string, std::string, std::vector<u64>>;
std::vector<ExchStageMergeSlot> merge_slots_from(const std::vector<PyMergeSlot>& slots) {
  std::vector<ExchStageMergeSlot> out(slots.size());
  for (size_t q = 0; q < slots.size(); ++q) {
    const std::string& h = std::get<0>(slots[q]);
    LOCUST_CHECK_ARG(h.size() == sizeof(SlotHeader), "a slot header holds 80 bytes");
    std::memcpy(&out[q].header, h.data(), sizeof(SlotHeader));
    out[q].records = records_from(std::get<1>(slots[q]), std::get<2>(slots[q]));
  }
  return out;
}
std::vector<u64> counts_of(const std::vector<KeyCount>& recs) {
  std::vector<u64> c(recs.size());
  for (size_t i = 0; i < c.size(); ++i) c[i] = recs[i].count;
  return c;
}
// A report of the compact emit's stage entry point: (status, flags, n_out).
using PyMsg3 = std::tuple<i32, u32, u64>;
std::vector<ExchMsg3> msg3_from(const std::vector<PyMsg3>& in) {
  std::vector<ExchMsg3> out(in.size());
  for (size_t q = 0; q < in.size(); ++q) {
    out[q] = ExchMsg3{};
    out[q].status = std::get<0>(in[q]);
    out[q].flags = std::get<1>(in[q]);
    out[q].n_out = std::get<2>(in[q]);
  }
  return out;
}

// ---- stage entry points of the dictionary kernels (locust/dict_stage.hpp) ----
DictStageCounters stage_counters_from(const py::dict& d) {
  auto get = [&](const char* k) -> u64 { return d.contains(k) ? d[k].cast<u64>() : 0; };
  DictStageCounters c;
  c.num_records = (u32)get("num_records");
  c.map_tokens = (u32)get("map_tokens");
  c.num_unique = (u32)get("num_unique");
  c.overflow_lines = (u32)get("overflow_lines");
  c.truncated = (u32)get("truncated");
  c.num_newlines = (u32)get("num_newlines");
  c.max_key_len = (u32)get("max_key_len");
  c.flags = (u32)get("flags");
  c.total_count = get("total_count");
  return c;
}
py::dict stage_counters_dict(const DictStageCounters& c) {
  py::dict d;
  d["num_records"] = c.num_records;
  d["map_tokens"] = c.map_tokens;
  d["num_unique"] = c.num_unique;
  d["overflow_lines"] = c.overflow_lines;
  d["truncated"] = c.truncated;
  d["num_newlines"] = c.num_newlines;
  d["max_key_len"] = c.max_key_len;
  d["flags"] = c.flags;
  d["total_count"] = c.total_count;
  return d;
}
py::dict dict_dense_dict(const DictStageDense& r, bool part_build) {
  py::dict d;
  d["num_unique"] = r.num_unique;
  d["flags"] = r.flags;
  d["keys"] = blob_from_keys(r.keys.data(), r.keys.size());
  d["counts"] = r.counts;
  d["tail_intact"] = r.tail_intact;
  if (part_build) {
    d["uval"] = r.uval;
    d["urank"] = r.urank;
  } else {
    py::list table;
    for (const DictStageSlot& s : r.table)
      table.append(py::make_tuple(s.slot, s.id, blob_from_keys(&s.key, 1)));
    d["table"] = table;
  }
  return d;
}

}  // namespace

PYBIND11_MODULE(_locust, m) {
  m.doc() = "Locust-MI355X native engine (HIP/CDNA4 kernels, RCCL shuffle)";

  py::enum_<Backend>(m, "Backend").value("gpu", Backend::kGpu).value("cpu", Backend::kCpu);
  py::enum_<ReducePath>(m, "ReducePath")
      .value("lds", ReducePath::kLds)
      .value("global_", ReducePath::kGlobal);
  py::enum_<MapPath>(m, "MapPath").value("compat", MapPath::kCompat).value("fast", MapPath::kFast);
  py::enum_<SortPath>(m, "SortPath").value("radix", SortPath::kRadix).value("dict", SortPath::kDict);

  py::class_<JobConfig>(m, "JobConfig")
      .def(py::init<>())
      .def_readwrite("backend", &JobConfig::backend)
      .def_readwrite("device", &JobConfig::device)
      .def_readwrite("emits_per_line", &JobConfig::emits_per_line)
      .def_readwrite("max_key_len", &JobConfig::max_key_len)
      .def_readwrite("ngram", &JobConfig::ngram)
      .def_readwrite("delimiters", &JobConfig::delimiters)
      .def_readwrite("ref_compat", &JobConfig::ref_compat)
      .def_readwrite("reduce_path", &JobConfig::reduce_path)
      .def_readwrite("map_path", &JobConfig::map_path)
      .def_readwrite("sort_path", &JobConfig::sort_path)
      .def_readwrite("combine", &JobConfig::combine)
      .def_readwrite("check", &JobConfig::check)
      .def_readwrite("sync_plan", &JobConfig::sync_plan)
      .def_readwrite("chunk_bytes", &JobConfig::chunk_bytes)
      .def_readwrite("zero_copy_text", &JobConfig::zero_copy_text)
      .def_readwrite("graph", &JobConfig::graph)
      .def_readwrite("ref_timers", &JobConfig::ref_timers)
      .def_readwrite("hbm_share", &JobConfig::hbm_share);
  m.def("plan_device_pass", [](const JobConfig& cfg, u64 max_bytes, u64 max_lines, u64 cap_records,
                               u64 free_bytes) {
    const DevicePassPlan p = plan_device_pass(cfg, max_bytes, max_lines, cap_records, free_bytes);
    py::dict d;
    d["streaming"] = p.streaming;
    d["chunk_bytes"] = p.chunk_bytes;
    d["pass_bytes"] = p.pass_bytes;
    d["map_window"] = p.map_window;
    d["cap_lines"] = p.cap_lines;
    d["cap"] = p.cap;
    d["ucap"] = p.ucap;
    d["rcap"] = p.rcap;
    d["device_bytes"] = p.device_bytes;
    d["budget_bytes"] = p.budget_bytes;
    d["why"] = p.why;
    return d;
  }, py::arg("cfg"), py::arg("max_bytes"), py::arg("max_lines"), py::arg("cap_records") = 0,
        py::arg("free_bytes") = 0,
        "The HBM plan of an engine's device pass (no GPU needed): sizes and device bytes.");

  py::enum_<DistStrategy>(m, "DistStrategy")
      .value("auto", DistStrategy::kAuto)
      .value("shuffle", DistStrategy::kShuffle)
      .value("gather", DistStrategy::kGather)
      .value("local", DistStrategy::kLocal);
  py::class_<DistConfig>(m, "DistConfig")
      .def(py::init<>())
      .def_readwrite("job", &DistConfig::job)
      .def_readwrite("world", &DistConfig::world)
      .def_readwrite("samples_per_rank", &DistConfig::samples_per_rank)
      .def_readwrite("gather", &DistConfig::gather)
      .def_readwrite("strategy", &DistConfig::strategy)
      .def_readwrite("gather_max_records", &DistConfig::gather_max_records);

  py::class_<PyResult>(m, "Result")
      .def("entries", &PyResult::entries)
      .def("times", &PyResult::times)
      .def("format", &PyResult::format, py::arg("cpu_format") = false)
      .def("write_kiv", [](const PyResult& p, const std::string& path) { write_kiv_results(path, p.r); },
           py::arg("path"), "The results as the reference's 40-B KeyIntValuePair records.")
      .def_property_readonly("num_lines", [](const PyResult& p) { return p.r.num_lines; })
      .def_property_readonly("num_tokens", [](const PyResult& p) { return p.r.num_tokens; })
      .def_property_readonly("num_unique", [](const PyResult& p) { return p.r.num_unique; })
      .def_property_readonly("overflow_lines", [](const PyResult& p) { return p.r.overflow_lines; })
      .def_property_readonly("truncated", [](const PyResult& p) { return p.r.truncated; })
      .def_property_readonly("max_key_len", [](const PyResult& p) { return p.r.max_key_len; })
      .def_property_readonly("compact", [](const PyResult& p) { return p.r.entries.compact(); },
                             "entries are the device's compact records (kv.hpp)")
      .def_property_readonly("wire_bytes", [](const PyResult& p) { return p.r.entries.wire_bytes(); },
                             "bytes the device wrote for the entries (compact or 40-B records)")
      .def_static("from_compact", [](const std::vector<u64>& words,
                                     const std::vector<std::pair<u64, u64>>& segs, u64 val_base) {
        // host-side decoder test: segments (word offset, entries) over a word buffer
        auto buf = std::make_shared<std::vector<u64>>(words);
        std::vector<EntrySegment> sv;
        u64 n = 0;
        for (const auto& sg : segs) {
          LOCUST_CHECK_ARG(sg.first <= buf->size(), "segment beyond the words");
          sv.push_back({buf->data() + sg.first, sg.second});
          n += sg.second;
        }
        PyResult p;
        p.r.entries.adopt_compact(buf, std::move(sv), n);
        p.r.val_base = val_base;
        p.r.num_unique = n;
        return p;
      }, py::arg("words"), py::arg("segments"), py::arg("val_base") = 0)
      .def("top", [](const PyResult& p, u64 k) {
        LOCUST_CHECK_ARG(k >= 1, "top-k: k must be at least 1");
        py::gil_scoped_release nogil;
        return PyTopResult{top_result(p.r, k)};
      }, py::arg("k"), "The host selection (any k): the top k entries by count, rank order.");

  py::class_<PyTopResult>(m, "TopResult")
      .def("entries", &PyTopResult::entries)
      .def("times", &PyTopResult::times)
      .def("format", &PyTopResult::format, py::arg("cpu_format") = false)
      .def_property_readonly("k", [](const PyTopResult& p) { return p.t.k; })
      .def_property_readonly("num_lines", [](const PyTopResult& p) { return p.t.num_lines; })
      .def_property_readonly("num_tokens", [](const PyTopResult& p) { return p.t.num_tokens; })
      .def_property_readonly("num_unique", [](const PyTopResult& p) { return p.t.num_unique; })
      .def_property_readonly("overflow_lines", [](const PyTopResult& p) { return p.t.overflow_lines; })
      .def_property_readonly("truncated", [](const PyTopResult& p) { return p.t.truncated; })
      .def_property_readonly("max_key_len", [](const PyTopResult& p) { return p.t.max_key_len; })
      .def_property_readonly("chunks", [](const PyTopResult& p) { return p.t.chunks; })
      .def_property_readonly("select_ms", [](const PyTopResult& p) { return p.t.select_ms; })
      .def_property_readonly("wire_bytes", [](const PyTopResult& p) { return p.t.wire_bytes; },
                             "bytes the device wrote to host memory for the result");
  py::class_<PyIndexResult>(m, "IndexResult", py::dynamic_attr())
      .def("entries", &PyIndexResult::entries)
      .def("postings", &PyIndexResult::postings)
      .def("postings_bytes", &PyIndexResult::postings_bytes)
      .def("lines", &PyIndexResult::lines, py::arg("key"), py::arg("unique") = false)
      .def("_search", &PyIndexResult::search, py::arg("queries"), py::arg("any"),
           py::arg("rank") = py::none(), py::arg("wildcard") = false,
           py::arg("within") = std::vector<u64>(),
           py::arg("exclude") = std::vector<std::vector<std::string>>(),
           py::arg("glob") = false, py::arg("ignore_case") = false, py::arg("show") = py::none(),
           py::arg("fuzzy") = false, py::arg("regex") = false, py::arg("tally") = py::none(),
           py::arg("files") = std::vector<std::vector<u32>>(), py::arg("by_file") = 0,
           "The host evaluation of all/any queries (any[i]: query i's mode) over this index.")
      .def("times", &PyIndexResult::times)
      .def("segments", [](const PyIndexResult& p) { return segment_rows(p.x.segment_table()); },
           "The index's files: [(id, first_line, base, lines)].")
      .def("format", &PyIndexResult::format)
      .def_property_readonly("first_line", [](const PyIndexResult& p) { return p.x.first_line; })
      .def_property_readonly("num_lines", [](const PyIndexResult& p) { return p.x.words.num_lines; })
      .def_property_readonly("num_tokens", [](const PyIndexResult& p) { return p.x.words.num_tokens; })
      .def_property_readonly("num_unique", [](const PyIndexResult& p) { return p.x.words.num_unique; })
      .def_property_readonly("overflow_lines",
                             [](const PyIndexResult& p) { return p.x.words.overflow_lines; })
      .def_property_readonly("truncated", [](const PyIndexResult& p) { return p.x.words.truncated; })
      .def_property_readonly("max_key_len", [](const PyIndexResult& p) { return p.x.words.max_key_len; })
      .def_property_readonly("index_ms", [](const PyIndexResult& p) { return p.x.index_ms; })
      .def_property_readonly("wire_bytes", [](const PyIndexResult& p) { return p.x.wire_bytes; },
                             "bytes the device wrote to host memory for the result");
  py::class_<PySearchResult>(m, "SearchResult", py::dynamic_attr())
      .def("lines", &PySearchResult::lines, py::arg("i"))
      .def("hits", &PySearchResult::hits, "the number of lines of every query")
      .def("term_counts", &PySearchResult::term_counts, py::arg("i"))
      .def("scores", &PySearchResult::scores, py::arg("i"),
           "ranked: the scores of lines(i), in the same order; unranked: empty")
      .def("matches", &PySearchResult::matches,
           "the number of matching lines of every query (unranked: hits())")
      .def_property_readonly("rank_k", [](const PySearchResult& p) { return p.r.rank_k; },
                             "the batch's K; 0: unranked")
      .def("times", &PySearchResult::times)
      .def("format", &PySearchResult::format, py::arg("mark") = false,
           "the CLI's result lines (mark: the shown spans between >> and <<)")
      .def("text", &PySearchResult::text, py::arg("i"),
           "show: the shown bytes of every entry of query i; without show: empty")
      .def("spans", &PySearchResult::spans, py::arg("i"),
           "show: per entry of query i its (start, len, mask) spans; without show: empty")
      .def("text_off", &PySearchResult::text_off,
           "show: [entries + 1] byte offsets of the entries' texts, in result order")
      .def("span_off", &PySearchResult::span_off,
           "show: [entries + 1] span offsets of the entries, in result order")
      .def_property_readonly("show_bytes", [](const PySearchResult& p) { return p.r.show_bytes; },
                             "the batch's N; 0: no show")
      .def_property_readonly("show_ms", [](const PySearchResult& p) { return p.r.show_ms; })
      .def("tally", &PySearchResult::tally, py::arg("i"),
           "tally: query i's most frequent words, [(key bytes, count)]; without tally: empty")
      .def("files", &PySearchResult::files, py::arg("i"),
           "by_file: the file id of every line of lines(i); otherwise empty")
      .def("local_lines", &PySearchResult::local_lines, py::arg("i"),
           "by_file: the file-local number of every line of lines(i); otherwise empty")
      .def("file_hits", &PySearchResult::file_hits, py::arg("i"),
           "by_file / count_only: [(file id, lines)] of query i, ids ascending; otherwise empty")
      .def_property_readonly("by_file", [](const PySearchResult& p) { return p.r.by_file; },
                             "0: no answers by file; 1: by_file; 2: count_only")
      .def_property_readonly("by_file_ms", [](const PySearchResult& p) { return p.r.by_file_ms; })
      .def("tally_words", &PySearchResult::tally_words,
           "tally: per query the words with count > 0 on its returned lines")
      .def("tally_tokens", &PySearchResult::tally_tokens,
           "tally: per query the emitted tokens of its returned lines")
      .def_property_readonly("tally_k", [](const PySearchResult& p) { return p.r.tally_k; },
                             "the batch's K; 0: no tally")
      .def_property_readonly("tally_ms", [](const PySearchResult& p) { return p.r.tally_ms; })
      .def_property_readonly("tallied", [](const PySearchResult& p) { return p.r.tallied; },
                             "tally: pair words the device stage sorted (0: the host evaluation)")
      .def_property_readonly("cut_lines", [](const PySearchResult& p) { return p.r.cut_lines; },
                             "show: entries whose line was longer than N")
      .def_property_readonly("span_count",
                             [](const PySearchResult& p) { return p.r.spans.size() / 3; },
                             "show: the spans of all entries")
      .def_property_readonly("queries", [](const PySearchResult& p) { return p.r.queries.size(); })
      .def_property_readonly("first_line", [](const PySearchResult& p) { return p.r.first_line; })
      .def_property_readonly("num_lines", [](const PySearchResult& p) { return p.r.num_lines; })
      .def_property_readonly("num_tokens", [](const PySearchResult& p) { return p.r.num_tokens; })
      .def_property_readonly("num_unique", [](const PySearchResult& p) { return p.r.num_unique; })
      .def_property_readonly("overflow_lines",
                             [](const PySearchResult& p) { return p.r.overflow_lines; })
      .def_property_readonly("truncated", [](const PySearchResult& p) { return p.r.truncated; })
      .def_property_readonly("max_key_len", [](const PySearchResult& p) { return p.r.max_key_len; })
      .def_property_readonly("index_ms", [](const PySearchResult& p) { return p.r.index_ms; })
      .def_property_readonly("search_ms", [](const PySearchResult& p) { return p.r.search_ms; })
      .def_property_readonly("walked", [](const PySearchResult& p) { return p.r.walked; },
                             "list elements the device's hit stage walked for the batch: the sum "
                             "of the queries' bounds (0: evaluated on the host)")
      .def_property_readonly("restricted", [](const PySearchResult& p) { return p.r.restricted; },
                             "hits the device's restrict stage removed under the batch's file "
                             "sets (0: no file set, or evaluated on the host)")
      .def("segments", [](const PySearchResult& p) {
        IndexSegments t;
        t.reset(p.r.first_line, p.r.num_lines);
        if (!p.r.segments.empty()) t.segs = p.r.segments;
        return segment_rows(t);
      }, "The files the batch was answered under: [(id, first_line, base, lines)].")
      .def_property_readonly("merged", [](const PySearchResult& p) { return p.r.merged; },
                             "list elements the device merged for prefix terms")
      .def_property_readonly("wire_bytes", [](const PySearchResult& p) { return p.r.wire_bytes; },
                             "bytes the device wrote to host memory for the result");
  m.attr("kSearchMaxQueries") = kSearchMaxQueries;
  m.attr("kSearchMaxTerms") = kSearchMaxTerms;
  m.attr("kCorpusMaxFiles") = kCorpusMaxFiles;
  // engine.hpp "corpus": the table's arithmetic alone (tests): ops are ("append", lines,
  // new_file) and ("drop", lines); returns per op the table as [(id, first_line, base, lines)]
  // and, for a drop, the dropped files (an append: 0); all_steps = false: the last op's only
  m.def("segment_ops", [](u64 first_line, u64 lines,
                          const std::vector<std::tuple<std::string, u64, bool>>& ops,
                          bool all_steps) {
    IndexSegments t;
    t.reset(first_line, lines);
    std::vector<std::pair<std::vector<std::tuple<u32, u64, u64, u64>>, u64>> out;
    if (all_steps || ops.empty()) out.emplace_back(segment_rows(t), 0);
    for (const auto& op : ops) {
      u64 gone = 0;
      if (std::get<0>(op) == "append")
        t.append(std::get<1>(op), std::get<2>(op));
      else
        gone = t.drop(std::get<1>(op));
      if (all_steps || &op == &ops.back()) out.emplace_back(segment_rows(t), gone);
    }
    return out;
  }, py::arg("first_line"), py::arg("lines"), py::arg("ops"), py::arg("all_steps") = true);
  m.def("segment_locate", [](const std::vector<std::tuple<u32, u64, u64, u64>>& rows, u64 line) {
    IndexSegments t;
    u64 n = 0;
    for (const auto& r : rows) {
      t.segs.push_back(IndexSegment{std::get<0>(r), std::get<1>(r), std::get<2>(r)});
      n += std::get<3>(r);
    }
    t.first_line = rows.empty() ? 0 : std::get<1>(rows[0]);
    t.num_lines = n;
    const size_t o = t.locate(line);
    return py::make_tuple(t.segs[o].id, line - t.segs[o].first_line + t.segs[o].base);
  }, py::arg("table"), py::arg("line"), "(id, local line) of a global line under a table");
  m.attr("kShowMaxBytes") = kShowMaxBytes;
  m.attr("kRankMaxEmits") = kRankMaxEmits;
  m.attr("kTopKMax") = kTopKMax;
  m.attr("kMaxNgram") = kMaxNgram;
  m.attr("kTopKTile") = kTopKTile;

  py::class_<PyGpuEngine>(m, "GpuEngine")
      .def(py::init<const JobConfig&, u64, u64>(), py::arg("cfg"), py::arg("max_bytes"),
           py::arg("max_lines"))
      .def("run", &PyGpuEngine::run)
      .def("load", &PyGpuEngine::load)
      .def("run_loaded", &PyGpuEngine::run_loaded)
      .def("stats", &PyGpuEngine::stats)
      .def("partition_map", [](PyGpuEngine& e) {
        std::vector<u64> lo;
        const bool tuned = e.engine().partition_map(&lo);
        return py::make_tuple(tuned, lo);
      }, "(tuned, the kDictParts + 1 range starts) after any background retune")
      .def("set_partition_map", [](PyGpuEngine& e, const std::vector<u64>& lo) {
        return e.engine().set_partition_map(lo);
      }, py::arg("lo"))
      .def("run_text", &PyGpuEngine::run_text, py::arg("text"))
      .def("run_file", &PyGpuEngine::run_file, py::arg("path"),
           "Stream a file through this (streaming) engine, piece by piece.")
      .def("map_stage", &PyGpuEngine::map_stage)
      .def("reduce_stage", &PyGpuEngine::reduce_stage)
      .def("sort_keys", &PyGpuEngine::sort_keys, py::arg("keys"), py::arg("counts") = py::none())
      .def("compact_slots", &PyGpuEngine::compact_slots)
      .def("reduce_sorted", &PyGpuEngine::reduce_sorted)
      .def("merge_runs", &PyGpuEngine::merge_runs)
      .def("run_top", &PyGpuEngine::run_top, py::arg("text"), py::arg("k"),
           "WordCount of text, top k by count selected on the device (k <= kTopKMax).")
      .def("run_top_text", &PyGpuEngine::run_top_text, py::arg("text"), py::arg("k"))
      .def("run_top_file", &PyGpuEngine::run_top_file, py::arg("path"), py::arg("k"))
      .def("run_index", &PyGpuEngine::run_index, py::arg("text"), py::arg("first_line") = 0,
           "WordCount of text and its inverted index (word -> lines), built on the device.")
      .def("run_index_text", &PyGpuEngine::run_index_text, py::arg("text"),
           py::arg("first_line") = 0)
      .def("run_search", &PyGpuEngine::run_search, py::arg("text"), py::arg("queries"),
           py::arg("any"), py::arg("first_line") = 0, py::arg("rank") = py::none(),
           py::arg("wildcard") = false, py::arg("within") = std::vector<u64>(),
           py::arg("exclude") = std::vector<std::vector<std::string>>(),
           py::arg("glob") = false, py::arg("ignore_case") = false, py::arg("show") = py::none(),
           py::arg("fuzzy") = false, py::arg("regex") = false, py::arg("tally") = py::none(),
           py::arg("files") = std::vector<std::vector<u32>>(), py::arg("by_file") = 0,
           "WordCount of text, its index, and all/any queries answered on the device.")
      .def("run_search_text", &PyGpuEngine::run_search_text, py::arg("text"), py::arg("queries"),
           py::arg("any"), py::arg("first_line") = 0, py::arg("rank") = py::none(),
           py::arg("wildcard") = false, py::arg("within") = std::vector<u64>(),
           py::arg("exclude") = std::vector<std::vector<std::string>>(),
           py::arg("glob") = false, py::arg("ignore_case") = false, py::arg("show") = py::none(),
           py::arg("fuzzy") = false, py::arg("regex") = false, py::arg("tally") = py::none(),
           py::arg("files") = std::vector<std::vector<u32>>(), py::arg("by_file") = 0)
      .def("search_resident", &PyGpuEngine::search_resident, py::arg("queries"), py::arg("any"),
           py::arg("rank") = py::none(), py::arg("wildcard") = false,
           py::arg("within") = std::vector<u64>(),
           py::arg("exclude") = std::vector<std::vector<std::string>>(),
           py::arg("glob") = false, py::arg("ignore_case") = false, py::arg("show") = py::none(),
           py::arg("fuzzy") = false, py::arg("regex") = false, py::arg("tally") = py::none(),
           py::arg("files") = std::vector<std::vector<u32>>(), py::arg("by_file") = 0,
           "Another batch from the index the last run_index / run_search left on the device.")
      .def("segments", &PyGpuEngine::segments,
           "The resident index's files: [(id, first_line, base, lines)].")
      .def("append_index", &PyGpuEngine::append_index, py::arg("text"), py::arg("first_line"),
           py::arg("new_file") = false,
           "One more block of whole lines into the resident index, merged on the device.")
      .def("drop_index", &PyGpuEngine::drop_index, py::arg("lines"),
           "The oldest `lines` lines out of the resident index, compacted on the device.")
      .def("index_resident", &PyGpuEngine::index_resident,
           "The resident index downloaded (IndexResult), whatever it was built from.")
      .def("top_counts", &PyGpuEngine::top_counts, py::arg("records"), py::arg("k"),
           "The selection kernels alone over key-sorted (key, count) records.")
      .def_property_readonly("capacity", &PyGpuEngine::capacity);

  m.def("cpu_run", [](const JobConfig& cfg, const std::string& text) {
    CpuWordCount eng(cfg);
    return PyResult{eng.run(as_input(text))};
  });
  m.def("cpu_run_top", [](const JobConfig& cfg, const std::string& text, u64 k) {
    CpuWordCount eng(cfg);
    return PyTopResult{eng.run_top(as_input(text), k)};
  }, py::arg("cfg"), py::arg("text"), py::arg("k"));
  m.def("cpu_run_index", [](const JobConfig& cfg, const std::string& text, u64 first_line) {
    CpuWordCount eng(cfg);
    return PyIndexResult{eng.run_index(as_input(text, first_line)), cfg};
  }, py::arg("cfg"), py::arg("text"), py::arg("first_line") = 0);
  py::class_<IndexAppend>(m, "IndexAppend")
      .def_readonly("block_lines", &IndexAppend::block_lines)
      .def_readonly("block_tokens", &IndexAppend::block_tokens)
      .def_readonly("block_unique", &IndexAppend::block_unique)
      .def_readonly("num_lines", &IndexAppend::num_lines)
      .def_readonly("num_tokens", &IndexAppend::num_tokens)
      .def_readonly("num_unique", &IndexAppend::num_unique)
      .def_readonly("fresh_words", &IndexAppend::fresh_words)
      .def_readonly("index_ms", &IndexAppend::index_ms)
      .def_readonly("append_ms", &IndexAppend::append_ms)
      .def_readonly("store_bytes", &IndexAppend::store_bytes)
      .def_readonly("files", &IndexAppend::files)
      .def("times", [](const IndexAppend& a) {
        py::dict d;
        d["h2d_ms"] = a.times.h2d_ms;
        d["map_ms"] = a.times.map_ms;
        d["process_ms"] = a.times.process_ms;
        d["reduce_ms"] = a.times.reduce_ms;
        d["gpu_ms"] = a.times.gpu_ms;
        d["wall_ms"] = a.times.wall_ms;
        d["index_ms"] = a.index_ms;
        d["append_ms"] = a.append_ms;
        return d;
      });
  py::class_<IndexDrop>(m, "IndexDrop")
      .def_readonly("dropped_lines", &IndexDrop::dropped_lines)
      .def_readonly("dropped_tokens", &IndexDrop::dropped_tokens)
      .def_readonly("dropped_words", &IndexDrop::dropped_words)
      .def_readonly("dropped_bytes", &IndexDrop::dropped_bytes)
      .def_readonly("dropped_overflow_lines", &IndexDrop::dropped_overflow_lines)
      .def_readonly("dropped_truncated", &IndexDrop::dropped_truncated)
      .def_readonly("dropped_files", &IndexDrop::dropped_files)
      .def_readonly("first_line", &IndexDrop::first_line)
      .def_readonly("num_lines", &IndexDrop::num_lines)
      .def_readonly("num_tokens", &IndexDrop::num_tokens)
      .def_readonly("num_unique", &IndexDrop::num_unique)
      .def_readonly("drop_ms", &IndexDrop::drop_ms)
      .def_readonly("store_bytes", &IndexDrop::store_bytes);
  m.def("trim_index", [](const PyIndexResult& x, u64 lines, u64 overflow_lines, u64 truncated) {
    py::gil_scoped_release nogil;
    return PyIndexResult{trim_index(x.x, lines, overflow_lines, truncated), x.cfg};
  }, py::arg("x"), py::arg("lines"), py::arg("overflow_lines") = 0, py::arg("truncated") = 0,
        "The index of x's text without its first `lines` lines (the dropped lines' statistics "
        "are the caller's to supply).");
  m.def("merge_index", [](const PyIndexResult& a, const PyIndexResult& b, bool new_file) {
    py::gil_scoped_release nogil;
    return PyIndexResult{merge_index(a.x, b.x, new_file), a.cfg};
  }, py::arg("a"), py::arg("b"), py::arg("new_file") = false,
        "The index of a's text followed by b's (b.first_line == a.first_line + a's lines).");
  // the host evaluation over an index and the text it was built from (every mode)
  m.def("search_index_text", [](const PyIndexResult& x, const std::string& text,
                                const std::vector<std::vector<std::string>>& queries,
                                const std::vector<int>& any, const py::object& rank, bool wildcard,
                                const std::vector<u64>& within,
                                const std::vector<std::vector<std::string>>& exclude, bool glob,
                                bool ignore_case, const py::object& show, bool fuzzy, bool regex,
                                const py::object& tally,
                        const std::vector<std::vector<u32>>& files, u32 by_file) {
    const std::vector<SearchQuery> q =
        to_queries(x.cfg, queries, any, wildcard, within, exclude, glob, fuzzy, regex, files);
    const u64 k = to_rank(rank), n = to_show(show), tk = to_tally(tally);
    py::gil_scoped_release nogil;
    return PySearchResult{
        search_index(x.x, as_input(text, x.x.first_line), q, x.cfg, k, ignore_case, n, tk, by_file)};
  });
  m.def("split_blocks", [](const std::string& text, u64 block_bytes, u64 first_line) {
    std::vector<std::tuple<u64, u64, u64, u64>> out;
    const TextInput in = as_input(text, first_line);
    for (const TextInput& b : split_blocks(in, block_bytes))
      out.emplace_back((u64)(b.data - in.data), b.bytes, b.num_lines, b.first_line);
    return out;
  }, py::arg("text"), py::arg("block_bytes"), py::arg("first_line") = 0,
        "Line-aligned blocks of at most block_bytes: [(offset, bytes, lines, first_line)].");
  m.def("cpu_run_search", [](const JobConfig& cfg, const std::string& text,
                             const std::vector<std::vector<std::string>>& queries,
                             const std::vector<int>& any, u64 first_line,
                             const py::object& rank, bool wildcard,
                             const std::vector<u64>& within,
                             const std::vector<std::vector<std::string>>& exclude, bool glob,
                        bool ignore_case, const py::object& show, bool fuzzy, bool regex,
                        const py::object& tally,
                        const std::vector<std::vector<u32>>& files, u32 by_file) {
    CpuWordCount eng(cfg);
    return PySearchResult{eng.run_search(as_input(text, first_line),
                                         to_queries(cfg, queries, any, wildcard, within, exclude, glob, fuzzy, regex, files),
                                         to_rank(rank), ignore_case, to_show(show),
                                         to_tally(tally), by_file)};
  }, py::arg("cfg"), py::arg("text"), py::arg("queries"), py::arg("any"),
        py::arg("first_line") = 0, py::arg("rank") = py::none(), py::arg("wildcard") = false,
        py::arg("within") = std::vector<u64>(),
           py::arg("exclude") = std::vector<std::vector<std::string>>(),
           py::arg("glob") = false, py::arg("ignore_case") = false, py::arg("show") = py::none(),
           py::arg("fuzzy") = false, py::arg("regex") = false, py::arg("tally") = py::none(),
           py::arg("files") = std::vector<std::vector<u32>>(), py::arg("by_file") = 0);
  m.def("make_search_expr", [](const JobConfig& cfg, const std::string& expr, bool wildcard,
                               bool glob, bool fuzzy, bool regex) {
    // engine.hpp "boolean expressions": the parsed query's parts (tests, tools)
    const SearchQuery q = make_search_expr(expr, cfg, wildcard, glob, fuzzy, regex);
    py::dict d;
    py::list terms, kinds, truth;
    for (size_t t = 0; t < q.terms.size(); ++t) {
      terms.append(py::bytes(q.terms[t]));
      kinds.append(q.is_regex(t) ? "regex" : q.fuzzy_budget(t) ? "fuzzy" : q.is_pattern(t) ? "pattern"
                   : q.is_prefix(t)  ? "prefix" : "plain");
    }
    for (const u32 w : q.truth) truth.append(w);
    d["expr"] = py::bytes(q.expr);
    d["terms"] = terms;
    d["kinds"] = kinds;
    d["truth"] = truth;
    d["excluded"] = q.excluded;
    return d;
  }, py::arg("cfg"), py::arg("expr"), py::arg("wildcard") = false, py::arg("glob") = false,
        py::arg("fuzzy") = false, py::arg("regex") = false,
        "The `expr` query of an expression: its text with blanks collapsed, its distinct terms in "
        "order of first occurrence, their kinds and the 8 x u32 truth table; throws for every "
        "refused expression.");
  m.attr("kExprMaxDepth") = kExprMaxDepth;
  m.def("compile_regex", [](const std::string& source, bool ignore_case) {
    return compile_regex(source, ignore_case);
  }, py::arg("source"), py::arg("ignore_case") = false,
        "A regex term's compiled program (engine.hpp \"regex terms\"; device/regex.hpp: first, "
        "last, nullable, positions, follow[32], B[256]); throws for every refused source.");
  m.def("make_search_query", [](const std::vector<std::string>& terms, bool wildcard, bool glob,
                                bool fuzzy, bool regex) {
    // how the terms of a query read (tests, tools): (bytes, kind) per term
    const SearchQuery q =
        make_search_query(terms, SearchMode::kAll, wildcard, 0, {}, glob, fuzzy, regex);
    py::list out;
    for (size_t t = 0; t < q.terms.size(); ++t)
      out.append(py::make_tuple(py::bytes(q.terms[t]),
                                q.is_regex(t)        ? "regex"
                                : q.fuzzy_budget(t)  ? "fuzzy"
                                : q.is_pattern(t)    ? "pattern"
                                : q.is_prefix(t)     ? "prefix"
                                                     : "plain"));
    return out;
  }, py::arg("terms"), py::arg("wildcard") = false, py::arg("glob") = false,
        py::arg("fuzzy") = false, py::arg("regex") = false,
        "The terms of a query as make_search_query reads them: (bytes, kind) per term.");
  m.attr("kRegexMaxDepth") = kRegexMaxDepth;
  m.attr("kRegexMaxSource") = kRegexMaxSource;
  m.attr("kRegexMaxPos") = kRegexMaxPos;
  m.def("check_search_show", &check_search_show, py::arg("show"), py::arg("text_bytes"),
        "Throws unless show is 0 or 1 <= N <= kShowMaxBytes over a window of < 2^32 bytes.");
  m.def("validate_show", [](const std::vector<std::string>& terms, const std::vector<u32>& lines,
                            const std::vector<u64>& text_lens, const std::vector<u32>& spans,
                            const std::vector<u64>& span_off, u32 show) {
    // validate_search over a one-query unranked result made of these parts (tests)
    SearchResult r;
    r.queries.push_back(make_search_query(terms, SearchMode::kAny, false));
    r.lines = lines;
    r.offsets = {0, lines.size()};
    r.matches = {lines.size()};
    r.num_lines = lines.empty() ? 0 : (u64)lines.back() + 1;
    r.term_counts.assign(kSearchMaxTerms, 0);
    r.show_bytes = show;
    r.text_off.assign(1, 0);
    for (const u64 l : text_lens) r.text_off.push_back(r.text_off.back() + l);
    r.text.assign((size_t)r.text_off.back(), 'x');
    r.spans = spans;
    r.span_off = span_off;
    validate_search(r);
  }, py::arg("terms"), py::arg("lines"), py::arg("text_lens"), py::arg("spans"),
        py::arg("span_off"), py::arg("show"));
  m.def("check_search_tally", &check_search_tally, py::arg("tally"),
        "Throws unless tally is 0 or 1 <= K <= kTopKMax.");
  m.def("tally_key_split", [](u64 n, u64 tokens) {
    const TallyKeySplit ks = tally_key_split(n, tokens);
    return py::make_tuple(ks.r, ks.c, ks.cmask);
  }, py::arg("n"), py::arg("tokens"),
        "The tally's rank-key split (r, c, cmask) for n index words and `tokens` pair words; "
        "throws when tokens >= 2^32 or c + r > 54.");
  m.def("validate_tally", [](const std::vector<std::string>& terms, const std::vector<u32>& lines,
                             u64 k, const std::vector<std::pair<std::string, u64>>& words,
                             u64 tally_words, u64 tally_tokens) {
    // validate_search over a one-query unranked result with these tallied words (tests)
    SearchResult r;
    r.queries.push_back(make_search_query(terms, SearchMode::kAny, false));
    r.lines = lines;
    r.offsets = {0, lines.size()};
    r.matches = {lines.size()};
    r.num_lines = lines.empty() ? 0 : (u64)lines.back() + 1;
    r.term_counts.assign(kSearchMaxTerms, 0);
    r.tally_k = k;
    for (const auto& w : words) {
      r.tally_keys.push_back(to_key(w.first));
      r.tally_counts.push_back(w.second);
    }
    r.tally_off = {0, words.size()};
    r.tally_words = {tally_words};
    r.tally_tokens = {tally_tokens};
    validate_search(r);
  }, py::arg("terms"), py::arg("lines"), py::arg("k"), py::arg("words"), py::arg("tally_words"),
        py::arg("tally_tokens"));
  m.def("check_search_merge", &check_search_merge, py::arg("queries"), py::arg("elements"),
        "Throws when a device batch's prefix terms would merge 2^32 list elements or more.");
  m.def("cpu_map_stage", [](const JobConfig& cfg, const std::string& text) {
    CpuWordCount eng(cfg);
    std::vector<py::bytes> out;
    for (const auto& k : eng.run_map_stage(as_input(text), nullptr)) out.emplace_back(key_to_string(k));
    return out;
  });
  m.def("radix_schedule", [](u32 act) {
    std::vector<u32> ws(kKeyWords), ps(kKeyBytes);
    for (int w = 0; w < kKeyWords; ++w) ws[w] = word_src(act, w);
    for (int p = 0; p < kKeyBytes; ++p) ps[p] = pass_src(act, p);
    return py::make_tuple(ws, ps, final_src(act));
  }, py::arg("act"),
        "The device-wide radix sort's buffer schedule for a mask of live digit positions: "
        "(word_src[4], pass_src[32], final_src), the functions its kernels call.");
  m.def("run_multi_schedule", &run_multi_schedule, py::arg("text"), py::arg("schedule"),
        py::arg("comm") = "auto",
        "Several jobs back to back on the same in-process ranks; [(Result, info)] of rank 0.");
  m.def("run_multi", &run_multi, py::arg("text"), py::arg("cfg"), py::arg("comm") = "auto",
        "Multi-rank WordCount in this process (one thread per rank): an RCCL clique "
        "(ncclCommInitAll) when every rank has a GPU of its own, else loopback.");
  m.def("run_multi_file", &run_multi_file, py::arg("path"), py::arg("cfg"),
        py::arg("comm") = "auto",
        "Multi-rank WordCount of a file in this process: rank r reads only its own "
        "line-aligned byte range (pinned one-pass read, or streamed past one pass); "
        "returns (rank 0's result, per-rank info dicts).");
  m.def("file_shards", [](const std::string& path, int parts) {
    py::list out;
    for (const auto& r : file_shards(path, parts)) out.append(py::make_tuple(r.offset, r.bytes));
    return out;
  }, py::arg("path"), py::arg("parts"), "Line-aligned byte ranges (offset, bytes) of a file.");
  m.def("peer_access", &enable_peer_access, py::arg("devices"),
        "Enable peer access between every pair of the devices; returns the n x n matrix "
        "(row-major) of direct-access flags.");
  m.def("peer_access_row", &peer_access_row, py::arg("device"),
        "hipDeviceCanAccessPeer(device, d) for every visible device d.");
  m.def("device_count", &visible_device_count,
        "Visible GPUs (initialises the HIP runtime in this process).");
  m.def("local_comm_for", [](const DistConfig& cfg, const std::string& comm) {
    return resolve_local_comm(cfg, local_comm(comm)) == LocalComm::kRccl ? "rccl" : "loopback";
  }, py::arg("cfg"), py::arg("comm") = "auto");

  m.def(
      "gen_text",
      [](u64 lines, u64 bytes, u64 seed, u32 vocab, double zipf_s, u64 first_block, u32 threads) {
        GenSpec g;
        g.lines = lines;
        g.bytes = bytes;
        g.seed = seed;
        g.vocab = vocab;
        g.zipf_s = zipf_s;
        g.first_block = first_block;
        g.threads = threads;
        std::string out;
        {
          py::gil_scoped_release nogil;
          gen_text(g, &out);
        }
        return py::bytes(out);
      },
      py::arg("lines") = 0, py::arg("bytes") = 0, py::arg("seed") = 1, py::arg("vocab") = 50000,
      py::arg("zipf_s") = 1.0, py::arg("first_block") = 0, py::arg("threads") = 0,
      "Synthetic Hamlet-shaped text (deterministic in seed and 1,024-line block).");
  m.def("gen_vocabulary", [](u32 vocab, u64 seed) {
    std::vector<py::bytes> out;
    for (const auto& w : gen_vocabulary(vocab, seed)) out.emplace_back(w);
    return out;
  }, py::arg("vocab"), py::arg("seed") = 1);

  py::class_<HostText>(m, "HostText",
                       "Input text in pinned host memory (DMA without staging; any size).")
      .def(py::init<u64>(), py::arg("capacity"))
      .def_static(
          "from_bytes",
          [](const std::string& b) {
            auto t = std::make_unique<HostText>(b.size());
            std::memcpy(t->data(), b.data(), b.size());
            t->set_size(b.size(), count_lines(b.data(), b.size()));
            return t;
          },
          py::arg("data"))
      .def_static(
          "generate",
          [](u64 lines, u64 bytes, u64 seed, u32 vocab, double zipf_s, u64 first_block,
             u32 threads, u64 capacity) {
            GenSpec g;
            g.lines = lines;
            g.bytes = bytes;
            g.seed = seed;
            g.vocab = vocab;
            g.zipf_s = zipf_s;
            g.first_block = first_block;
            g.threads = threads;
            // lines mode: ~44 B per line on average, 100 B at most
            const u64 cap = capacity ? capacity : (bytes ? bytes : lines * 100 + 64);
            auto t = std::make_unique<HostText>(cap);
            u64 nl = 0, n = 0;
            {
              py::gil_scoped_release nogil;
              n = gen_text_into(g, t->data(), cap, &nl);
            }
            t->set_size(n, nl);
            return t;
          },
          py::arg("lines") = 0, py::arg("bytes") = 0, py::arg("seed") = 1,
          py::arg("vocab") = 50000, py::arg("zipf_s") = 1.0, py::arg("first_block") = 0,
          py::arg("threads") = 0, py::arg("capacity") = 0)
      .def_property_readonly("size", &HostText::size)
      .def_property_readonly("lines", &HostText::lines)
      .def_property_readonly("pinned", &HostText::pinned)
      .def("to_bytes", [](const HostText& t) { return py::bytes(t.data(), t.size()); });

  m.def(
      "device_string_selftest",
      [](const std::vector<std::string>& strings, const std::vector<int>& ints,
         const std::string& delims) {
        std::vector<StringTestOut> rows;
        {
          py::gil_scoped_release nogil;
          rows = run_string_selftest(strings, ints, delims);
        }
        py::list out;
        for (const auto& o : rows) {
          py::list offs;
          for (int k = 0; k < std::min(o.ntok, 8); ++k) offs.append(o.tok_off[k]);
          out.append(py::make_tuple(o.len, o.cmp_next, o.copy_len, py::bytes(o.copy), o.ntok,
                                    offs, std::string(o.itoa_buf)));
        }
        return out;
      },
      py::arg("strings"), py::arg("ints"), py::arg("delims"),
      "Run strlen/strcmp/strcpy_bounded/strtok_r/itoa on the GPU (one thread per string).");

  py::class_<PyDistRank>(m, "DistRank")
      .def(py::init<const DistConfig&, int, const std::string&, const std::string&, int, u64, u64,
                    double, int>(),
           py::arg("cfg"), py::arg("rank"), py::arg("comm"), py::arg("host"), py::arg("port"),
           py::arg("max_bytes"), py::arg("max_lines"), py::arg("timeout_s") = 300.0,
           py::arg("listen_fd") = -1)
      .def("add_engine", &PyDistRank::add_engine, py::arg("max_bytes"), py::arg("max_lines"))
      .def("use_engine", &PyDistRank::use_engine)
      .def_property_readonly("comm_count", &PyDistRank::comm_count)
      .def_property_readonly("comm_name", &PyDistRank::comm_name)
      .def("run", &PyDistRank::run, py::arg("shard"), py::arg("first_line") = 0)
      .def("load", &PyDistRank::load, py::arg("shard"), py::arg("first_line") = 0)
      .def("run_loaded", &PyDistRank::run_loaded)
      .def("load_text", &PyDistRank::load_text, py::arg("text"), py::arg("first_line") = 0,
           py::keep_alive<1, 2>())
      .def("set_strategy", &PyDistRank::set_strategy)
      .def("barrier", &PyDistRank::barrier)
      .def("allreduce_max", &PyDistRank::allreduce_max)
      .def("allgather_bytes", &PyDistRank::allgather_bytes)
      .def_property_readonly("rank", &PyDistRank::rank)
      .def_property_readonly("size", &PyDistRank::size);

  m.def("load_lines",
        [](const std::string& path, i64 start, i64 end, bool ref_compat) {
          LoadedText t = load_lines(path, start, end, ref_compat);
          return py::make_tuple(py::bytes(t.storage.data(), t.storage.size()), t.input.num_lines,
                                t.input.first_line, t.file_lines);
        },
        py::arg("path"), py::arg("line_start") = -1, py::arg("line_end") = -1,
        py::arg("ref_compat") = false);
  m.def("gpu_placement", [](const std::string& bdf, const std::string& sys_root) {
    const GpuPlacement pl = placement_for_bdf(bdf, sys_root);
    return py::make_tuple(pl.bdf, pl.numa_node, pl.cpus);
  }, py::arg("bdf"), py::arg("sys_root") = "/sys");
  m.def("parse_cpulist", &parse_cpulist);
  m.def("plan_rank_slices", [](u64 header, u64 region, u32 regions, const std::vector<int>& nodes,
                               u64 page) {
    py::list out;
    for (const auto& s : plan_rank_slices(header, region, regions, nodes, page))
      out.append(py::make_tuple(s.offset, s.bytes, s.node));
    return out;
  }, py::arg("header"), py::arg("region"), py::arg("regions"), py::arg("nodes"),
        py::arg("page") = 4096, "NUMA slices (offset, bytes, node) of a shared output segment");
  m.def("spans_numa_nodes", &spans_numa_nodes);
  // A shm segment placed by `plan` ([(offset, bytes, node)]): returns the node of each
  // page's first byte after the segment was reserved and touched (-1: unknown).
  m.def("shm_placement_probe", [](u64 bytes, const std::vector<std::tuple<u64, u64, int>>& plan) {
    std::vector<NumaSlice> pl;
    for (const auto& t : plan) pl.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t)});
    ShmSegment seg;
    seg.open(shm_segment_name(new_group_token(), 1), align_up(bytes, 4096), &pl);
    std::vector<int> nodes;
    for (u64 o = 0; o < seg.bytes(); o += 4096) {
      seg.data()[o] = 1;
      nodes.push_back(page_node(seg.data() + o));
    }
    seg.close();
    return nodes;
  }, py::arg("bytes"), py::arg("plan"));
  // the shared output segment (locust/shm.hpp), for host-side tests
  py::class_<ShmSegment>(m, "ShmSegment")
      .def(py::init([](const std::string& name, u64 bytes) {
             auto s = std::make_unique<ShmSegment>();
             s->open(name, bytes);
             return s;
           }),
           py::arg("name"), py::arg("bytes"))
      .def_property_readonly("bytes", &ShmSegment::bytes)
      .def_property_readonly("name", &ShmSegment::name)
      .def_property_readonly("linked", &ShmSegment::linked)
      .def("write", [](ShmSegment& s, u64 off, const std::string& b) {
        LOCUST_CHECK_ARG(off + b.size() <= s.bytes(), "write past the segment");
        std::memcpy(s.data() + off, b.data(), b.size());
      })
      .def("read", [](ShmSegment& s, u64 off, u64 n) {
        LOCUST_CHECK_ARG(off + n <= s.bytes(), "read past the segment");
        return py::bytes(s.data() + off, n);
      })
      .def("unlink", &ShmSegment::unlink)
      .def("close", &ShmSegment::close);
  m.def("dev_cache_stats", [] {  // the process-wide device block cache (devcache.hpp)
    size_t bytes = 0;
    const size_t n = dev_block_cached(&bytes);
    py::dict d;
    d["blocks"] = n;
    d["bytes"] = bytes;
    return d;
  });
  m.def("dev_cache_trim", &dev_block_trim);
  m.def("shm_segment_name", &shm_segment_name);
  m.def("shm_segment_bytes", &shm_segment_bytes);
  m.def("next_segment_gen", &next_segment_gen);
  m.def("new_group_token", &new_group_token);
  m.def("file_source_chunks",  // the streamed file source's chunks (tests)
        [](const std::string& path, u64 cap, u32 threads) {
          auto src = open_file_source(path, threads);
          std::vector<char> buf(cap);
          py::list parts;
          for (u64 n; (n = src->next(buf.data(), cap)) != 0;) parts.append(py::bytes(buf.data(), n));
          return py::make_tuple(parts, src->lines());
        },
        py::arg("path"), py::arg("cap"), py::arg("threads") = 2);
  m.def("text_window",  // the in-memory window (the loader's reference semantics)
        [](const std::string& text, i64 start, i64 end, bool ref_compat) {
          LoadedText t = text_from_buffer(text.data(), text.size(), start, end, ref_compat);
          return py::make_tuple(py::bytes(t.storage.data(), t.storage.size()), t.input.num_lines,
                                t.input.first_line, t.file_lines);
        },
        py::arg("text"), py::arg("line_start") = -1, py::arg("line_end") = -1,
        py::arg("ref_compat") = false);
  m.def("shard_bounds", [](const std::string& text, int parts) {
    TextInput in = as_input(text);
    py::list out;
    for (const auto& s : shard_text(in, parts))
      out.append(py::make_tuple((u64)(s.data - in.data), s.bytes, s.num_lines, s.first_line));
    return out;
  });
  m.def("strtok_r_tokens", &strtok_r_tokens, py::arg("line"), py::arg("delims") = std::string(kDefaultDelims));
  m.def("itoa", [](int n, int base) {
    char buf[40];
    return std::string(d_itoa(n, buf, base));
  });
  m.def("strcmp", [](const std::string& a, const std::string& b) { return d_strcmp(a.c_str(), b.c_str()); });
  m.def("part_map_build", [](const std::vector<std::pair<std::string, u64>>& keys, u32 max_distinct) {
    // Balanced partition map (locust/partmap.hpp) for sorted (key, count) pairs: the
    // tables plus the predicted largest partition work.
    std::vector<WordCountEntry> e(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
      e[i].key = to_key(keys[i].first);
      e[i].count = keys[i].second;
    }
    PartMapTables t;
    const u64 pred = part_map_from_entries(EntryList(std::vector<WordCountEntry>(e)), &t, max_distinct);
    py::dict d;
    d["lo"] = std::vector<u64>(t.lo, t.lo + kDictParts + 1);
    d["predicted_max"] = pred;
    std::vector<u32> part(e.size());  // partition of every input key
    for (size_t i = 0; i < e.size(); ++i) part[i] = part_map_lookup(t, e[i].key.w[0]);
    d["part"] = part;
    return d;
  }, py::arg("keys"), py::arg("max_distinct") = 1024);
  m.def("part_of_key", [](const std::vector<u64>& lo, const std::string& key) {
    LOCUST_CHECK_ARG(lo.size() == (size_t)kDictParts + 1, "lo needs kDictParts + 1 entries");
    return part_of_w0(lo.data(), to_key(key).w[0]);
  });
  m.def("pack_key", [](const std::string& s) {
    PackedKey k = to_key(s);
    return std::vector<u64>(k.w, k.w + kKeyWords);
  });
  // ---- the device shuffle's stages, each alone (locust/exch_stage.hpp; tests) ----
  m.attr("EXCH_SEND_OVERFLOW") = kExchSendOverflow;
  m.attr("EXCH_RECV_TRUNCATED") = kExchRecvTruncated;
  m.attr("EXCH_ABORT") = kExchAbort;
  m.attr("EXCH_TOO_MANY_SAMPLES") = kExchTooManySamples;
  m.attr("EXCH_GATHER_OVERFLOW") = kExchGatherOverflow;
  m.attr("EXCH_MAP_REDO") = kExchMapRedo;
  m.attr("EXCH_MAX_RANKS") = kExchMaxRanks;
  m.attr("EXCH_MAX_PLAN_SAMPLES") = kExchMaxPlanSamples;
  m.attr("SLOT_OK") = kSlotOk;
  m.attr("SLOT_FAILED") = kSlotFailed;
  m.attr("SLOT_REDO") = kSlotRedo;
  m.attr("EXCH_STAGE_PATTERN") = (u32)kExchStagePattern;
  m.def("ctr_dict_overflow_flag", &exch_stage_dict_overflow_flag);
  m.def("choose_splitters", [](const std::string& samples, u32 s, const std::vector<u64>& counts,
                               int parts) {
    const std::vector<PackedKey> smp = keys_from_blob(samples);
    LOCUST_CHECK_ARG(s >= 1 && parts >= 1 && smp.size() == counts.size() * (u64)s,
                     "need s samples per rank");
    const std::vector<PackedKey> sp = choose_splitters(smp, s, counts, parts);
    return blob_from_keys(sp.data(), sp.size());
  }, py::arg("samples"), py::arg("s"), py::arg("counts"), py::arg("parts"),
        "The host-staged shuffle's weighted-quantile splitters (dist.cpp; no GPU).");
  m.def("exch_plan_pack", [](u32 P, u32 S, const std::vector<i32>& status,
                             const std::vector<u64>& n_local, const std::string& samples,
                             const std::string& keys, const std::vector<u64>& counts,
                             u32 slot_records, u64 pack_cap) {
    const std::vector<PackedKey> smp = keys_from_blob(samples);
    const std::vector<KeyCount> recs = records_from(keys, counts);
    ExchStagePlan p;
    {
      py::gil_scoped_release nogil;
      p = exch_stage_plan_pack(P, S, status, n_local, smp, recs, slot_records, pack_cap);
    }
    return exch_plan_dict(p, P);
  }, py::arg("P"), py::arg("S"), py::arg("status"), py::arg("n_local"), py::arg("samples"),
        py::arg("keys"), py::arg("counts"), py::arg("slot_records"), py::arg("pack_cap") = 0,
        "launch_exch_plan + launch_exch_pack on free-standing messages and sorted records.");
  m.def("exch_pack", [](const std::vector<u64>& off, u32 flags, const std::string& keys,
                        const std::vector<u64>& counts, u32 slot_records, u64 pack_cap) {
    LOCUST_CHECK_ARG(off.size() >= 2 && off.size() <= (size_t)kExchMaxRanks + 1,
                     "exchange: bad shape");
    const u32 P = (u32)off.size() - 1;
    ExchCtl ctl{};
    for (size_t i = 0; i < off.size(); ++i) ctl.off[i] = off[i];
    ctl.flags = flags;
    for (u32 p = 0; p < P; ++p)
      if (off[p + 1] >= off[p]) ctl.max_bucket = std::max(ctl.max_bucket, off[p + 1] - off[p]);
    const std::vector<KeyCount> recs = records_from(keys, counts);
    ExchStagePlan p;
    {
      py::gil_scoped_release nogil;
      p = exch_stage_pack(ctl, P, recs, slot_records, pack_cap);
    }
    return exch_plan_dict(p, P);
  }, py::arg("off"), py::arg("flags"), py::arg("keys"), py::arg("counts"),
        py::arg("slot_records"), py::arg("pack_cap") = 0,
        "launch_exch_pack alone behind given bucket offsets (P + 1) and plan flags.");
  m.def("exch_sample", [](const std::string& keys, u32 S) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    std::vector<PackedKey> out;
    {
      py::gil_scoped_release nogil;
      out = exch_stage_sample(k, S);
    }
    return blob_from_keys(out.data(), out.size());
  }, py::arg("keys"), py::arg("S"), "launch_sample_keys of sorted keys -> S keys.");
  m.def("exch_header", [](const py::dict& ctr, const py::dict& tmpl, bool combined,
                          const std::string& keys, u32 S) {
    auto get = [](const py::dict& d, const char* k) -> u64 {
      return d.contains(k) ? d[k].cast<u64>() : 0;
    };
    ExchStageCounters c;
    c.flags = (u32)get(ctr, "flags");
    c.num_unique = (u32)get(ctr, "num_unique");
    c.num_records = (u32)get(ctr, "num_records");
    c.map_tokens = (u32)get(ctr, "map_tokens");
    c.overflow_lines = (u32)get(ctr, "overflow_lines");
    c.truncated = (u32)get(ctr, "truncated");
    c.max_key_len = (u32)get(ctr, "max_key_len");
    ExchMsg1 t{};
    t.status = tmpl.contains("status") ? tmpl["status"].cast<i32>() : 0;
    t.record_flags = (u32)get(tmpl, "record_flags");
    t.n_local = get(tmpl, "n_local");
    t.lines = get(tmpl, "lines");
    t.tokens = get(tmpl, "tokens");
    t.overflow_lines = get(tmpl, "overflow_lines");
    t.truncated = get(tmpl, "truncated");
    t.max_key_len = get(tmpl, "max_key_len");
    t.out_region = get(tmpl, "out_region");
    const std::vector<PackedKey> k = keys_from_blob(keys);
    ExchStageHeader h;
    {
      py::gil_scoped_release nogil;
      h = exch_stage_header(c, t, combined, k, S);
    }
    py::dict d;
    d["status"] = h.msg.status;
    d["record_flags"] = h.msg.record_flags;
    d["n_local"] = h.msg.n_local;
    d["lines"] = h.msg.lines;
    d["tokens"] = h.msg.tokens;
    d["overflow_lines"] = h.msg.overflow_lines;
    d["truncated"] = h.msg.truncated;
    d["max_key_len"] = h.msg.max_key_len;
    d["out_region"] = h.msg.out_region;
    d["samples"] = blob_from_keys(h.samples.data(), h.samples.size());
    d["tail_intact"] = h.tail_intact;
    return d;
  }, py::arg("ctr"), py::arg("tmpl"), py::arg("combined"), py::arg("keys"), py::arg("S"),
        "launch_exch_header: the written ExchMsg1, its S samples, and whether the bytes "
        "behind them are untouched.");
  m.def("exch_offsets", [](const std::string& keys, const std::string& splitters, u32 P) {
    const std::vector<PackedKey> k = keys_from_blob(keys), sp = keys_from_blob(splitters);
    py::gil_scoped_release nogil;
    return exch_stage_offsets(k, sp, P);
  }, py::arg("keys"), py::arg("splitters"), py::arg("P"),
        "launch_bucket_offsets of P - 1 splitters in sorted keys -> P + 1 offsets.");
  m.def("exch_roundtrip", [](const std::string& keys, const py::object& counts,
                             const std::vector<u64>& lo) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    std::vector<u64> c;
    if (!counts.is_none()) c = counts.cast<std::vector<u64>>();
    ExchStageRoundTrip r;
    {
      py::gil_scoped_release nogil;
      r = exch_stage_roundtrip(k, counts.is_none() ? nullptr : &c, lo);
    }
    py::dict d;
    d["packed_keys"] = blob_from_keys(r.packed.data(), r.packed.size());
    std::vector<u64> pc(r.packed.size());
    for (size_t i = 0; i < pc.size(); ++i) pc[i] = r.packed[i].count;
    d["packed_counts"] = pc;
    d["keys"] = blob_from_keys(r.keys.data(), r.keys.size());
    d["counts"] = r.counts;
    d["parts"] = py::bytes(reinterpret_cast<const char*>(r.parts.data()), r.parts.size());
    return d;
  }, py::arg("keys"), py::arg("counts"), py::arg("lo") = std::vector<u64>{},
        "launch_pack_records, then launch_unpack_records with the partition map `lo`.");
  m.def("exch_report", [](const std::vector<std::pair<i32, u64>>& headers, u32 slot_records,
                          u32 flags, u64 max_bucket, const std::vector<u64>& acc,
                          u32 gather_records) {
    std::vector<SlotHeader> hs(headers.size());
    for (size_t q = 0; q < hs.size(); ++q) {
      hs[q] = SlotHeader{};
      hs[q].status = headers[q].first;
      hs[q].record_flags = 3u;
      hs[q].n = headers[q].second;
      hs[q].slot_cap = slot_records;
    }
    ExchCtl ctl{};
    ctl.flags = flags;
    ctl.max_bucket = max_bucket;
    ExchStageReport r;
    {
      py::gil_scoped_release nogil;
      r = exch_stage_report(hs, slot_records, ctl, acc, gather_records);
    }
    py::dict d;
    d["status"] = r.msg.status;
    d["flags"] = r.msg.flags;
    d["max_bucket"] = r.msg.max_bucket;
    d["n_out"] = r.msg.n_out;
    d["total"] = r.msg.total;
    d["out_words"] = r.msg.out_words;
    d["pad"] = std::vector<u64>(r.msg.pad, r.msg.pad + 3);
    d["acc"] = r.acc;
    return d;
  }, py::arg("headers"), py::arg("slot_records"), py::arg("flags"), py::arg("max_bucket"),
        py::arg("acc"), py::arg("gather_records"),
        "launch_exch_report over P received (status, n) slot headers.");
  m.attr("MERGE_MAX_RECORDS") = kMergeMaxRecords;
  m.attr("MERGE_MAX_COUNT") = kMergeMaxCount;
  m.attr("MAX_SLOT_RANKS") = kMaxSlotRanks;
  m.def("slot_merge_fits", &slot_merge_fits, py::arg("nslots"), py::arg("slot_records"),
        py::arg("tokens"),
        "Whether the gather strategy's root may merge this many all-gathered slots holding "
        "this many tokens (slot.hpp; no GPU); otherwise the job takes the standard path.");
  m.def("exch_merge_slots", [](const std::vector<PyMergeSlot>& slots, u32 slot_records) {
    const std::vector<ExchStageMergeSlot> in = merge_slots_from(slots);
    ExchStageMerge r;
    {
      py::gil_scoped_release nogil;
      r = exch_stage_merge_slots(in, slot_records);
    }
    py::dict d;
    d["keys"] = blob_from_keys(r.out.data(), r.out.size());
    d["counts"] = counts_of(r.out);
    d["ctr"] = py::make_tuple(r.ctr.num_records, r.ctr.num_unique, r.ctr.total_count);
    d["ctr_out"] = py::make_tuple(r.ctr_out.num_records, r.ctr_out.num_unique,
                                  r.ctr_out.total_count);
    py::list hs;
    for (const SlotHeader& h : r.headers)
      hs.append(py::bytes(reinterpret_cast<const char*>(&h), sizeof h));
    d["headers"] = hs;
    d["tail_intact"] = r.tail_intact;
    return d;
  }, py::arg("slots"), py::arg("slot_records"),
        "launch_merge_slots over (header bytes, keys, counts) slots: the output records, "
        "(num_records, num_unique, total_count) of ctr and ctr_out, the copied headers.");
  m.def("exch_rank_slots", [](const std::vector<PyMergeSlot>& slots, u32 slot_records) {
    const std::vector<ExchStageMergeSlot> in = merge_slots_from(slots);
    ExchStageRank r;
    {
      py::gil_scoped_release nogil;
      r = exch_stage_rank_slots(in, slot_records);
    }
    py::dict d;
    d["keys"] = blob_from_keys(r.merged.data(), r.merged.size());
    d["counts"] = counts_of(r.merged);
    d["acc"] = r.acc;
    return d;
  }, py::arg("slots"), py::arg("slot_records"),
        "launch_merge_rank_slots: the whole merged array and the accumulator triples.");
  m.def("exch_emit_compact", [](const std::vector<PyMergeSlot>& slots, u32 slot_records,
                                const std::vector<PyMsg3>& msg3_all, const py::object& root_region,
                                u64 region, u32 regions, u64 region_records, u32 me,
                                u32 gather_records, u64 seq, int jobs, const py::object& slots2,
                                const py::object& msg3_all2) {
    LOCUST_CHECK_ARG(jobs == 1 || jobs == 2, "merge stage: 1 or 2 jobs");
    std::vector<ExchStageEmitJob> in(jobs);
    in[0].slots = merge_slots_from(slots);
    in[0].msg3 = msg3_from(msg3_all);
    if (jobs == 2) {
      LOCUST_CHECK_ARG(!slots2.is_none() && !msg3_all2.is_none(),
                       "merge stage: the second job needs slots2 and msg3_all2");
      in[1].slots = merge_slots_from(slots2.cast<std::vector<PyMergeSlot>>());
      in[1].msg3 = msg3_from(msg3_all2.cast<std::vector<PyMsg3>>());
    }
    const bool use_root = !root_region.is_none();
    const u64 root = use_root ? root_region.cast<u64>() : 0;
    std::vector<ExchStageEmit> r;
    {
      py::gil_scoped_release nogil;
      r = exch_stage_emit_compact(in, slot_records, use_root, root, region, regions,
                                  region_records, me, gather_records, seq);
    }
    py::list out;
    for (const ExchStageEmit& e : r) {
      py::dict d;
      d["dst"] = e.dst;
      d["stamps"] = e.stamps;
      d["done"] = e.done;
      d["acc"] = e.acc;
      out.append(d);
    }
    return out;
  }, py::arg("slots"), py::arg("slot_records"), py::arg("msg3_all"), py::arg("root_region"),
        py::arg("region"), py::arg("regions"), py::arg("region_records"), py::arg("me"),
        py::arg("gather_records"), py::arg("seq"), py::arg("jobs") = 1,
        py::arg("slots2") = py::none(), py::arg("msg3_all2") = py::none(),
        "launch_merge_rank_slots + launch_merge_emit_compact per job (the second on slots2 / "
        "msg3_all2, seq + 1, the same scratch): per job dst (with its guard), stamps, done "
        "and the accumulators.  msg3_all: (status, flags, n_out) per rank.");
  // ---- the dictionary kernels and the partition plan, each alone (locust/dict_stage.hpp) ----
  m.def("dict_constants", [] {
    py::dict d;
    for (const auto& kv : dict_stage_constants()) d[py::str(kv.first)] = kv.second;
    return d;
  }, "Kernel constants of dict.hip / partplan.hip by name (device/dict_consts.hpp; no GPU).");
  m.def("dict_valid_key", [](const std::string& key) {
    const std::vector<PackedKey> k = keys_from_blob(key);
    LOCUST_CHECK_ARG(k.size() == 1, "one 32-byte key");
    return dict_stage_valid_key(k[0].w);
  }, "Whether 32 bytes are a valid packed key: bytes, then NUL padding only (no GPU).");
  m.def("dict_insert", [](const std::string& keys, const py::object& counts, u32 d_n, u64 cap,
                          u64 table_slots, u32 ucap, u32 max_blocks) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    std::vector<u64> c;
    if (!counts.is_none()) c = counts.cast<std::vector<u64>>();
    DictStageDense r;
    {
      py::gil_scoped_release nogil;
      r = dict_stage_insert(k, counts.is_none() ? nullptr : &c, d_n, cap, table_slots, ucap,
                            max_blocks);
    }
    return dict_dense_dict(r, false);
  }, py::arg("keys"), py::arg("counts"), py::arg("d_n"), py::arg("cap"), py::arg("table_slots"),
        py::arg("ucap"), py::arg("max_blocks") = 1024,
        "launch_dict_insert on a zeroed table: num_unique, flags, the dense keys / counts "
        "[0, min(num_unique, ucap)), tail_intact and the occupied slots (slot, id, key).");
  m.def("dict_part_build", [](const std::string& keys, const py::object& counts,
                              const std::string& parts, u32 d_n, u64 cap, u32 ucap) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    std::vector<u64> c;
    if (!counts.is_none()) c = counts.cast<std::vector<u64>>();
    const std::vector<u8> p(parts.begin(), parts.end());
    DictStageDense r;
    {
      py::gil_scoped_release nogil;
      r = dict_stage_part_build(k, counts.is_none() ? nullptr : &c, p, d_n, cap, ucap);
    }
    return dict_dense_dict(r, true);
  }, py::arg("keys"), py::arg("counts"), py::arg("parts"), py::arg("d_n"), py::arg("cap"),
        py::arg("ucap"),
        "launch_dict_part_build: the dense view as dict_insert's, with uval / urank of the "
        "dense ids.");
  m.def("dict_rank", [](const std::string& keys, const py::object& counts, u32 d_u, u64 cap) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    std::vector<u64> c;
    if (!counts.is_none()) c = counts.cast<std::vector<u64>>();
    DictStageRank r;
    {
      py::gil_scoped_release nogil;
      r = dict_stage_rank(k, counts.is_none() ? nullptr : &c, d_u, cap);
    }
    py::dict d;
    d["rank"] = r.rank;
    d["val"] = r.val;
    d["tail_intact"] = r.tail_intact;
    return d;
  }, py::arg("keys"), py::arg("counts"), py::arg("d_u"), py::arg("cap"),
        "launch_rank_sort on zeroed rank / val: both whole arrays (cap entries).");
  m.def("dict_emit", [](const std::string& keys, const std::vector<u64>& counts,
                        const std::vector<u32>& rank, const std::vector<u64>& val,
                        const py::dict& ctr, u64 cap) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    const DictStageCounters c = stage_counters_from(ctr);
    DictStageEmit r;
    {
      py::gil_scoped_release nogil;
      r = dict_stage_emit(k, counts, rank, val, c, cap);
    }
    py::dict d;
    d["keys"] = blob_from_keys(r.records.data(), r.records.size());
    d["counts"] = counts_of(r.records);
    d["ctr_out"] = stage_counters_dict(r.ctr_out);
    d["tail_intact"] = r.tail_intact;
    d["untouched"] = r.untouched;
    return d;
  }, py::arg("keys"), py::arg("counts"), py::arg("rank"), py::arg("val"), py::arg("ctr"),
        py::arg("cap"),
        "launch_rank_emit: the records [0, min(num_unique, cap)), ctr_out field by field, "
        "whether the output behind the records (tail_intact) or all of it (untouched) still "
        "holds the pattern.");
  m.def("dict_scatter", [](const std::string& keys, const std::vector<u64>& counts,
                           const std::vector<u32>& rank, u32 d_u, u64 cap) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    DictStageScatter r;
    {
      py::gil_scoped_release nogil;
      r = dict_stage_scatter(k, counts, rank, d_u, cap);
    }
    py::dict d;
    d["keys"] = blob_from_keys(r.sorted.data(), r.sorted.size());
    d["counts"] = r.counts;
    d["tail_intact"] = r.tail_intact;
    return d;
  }, py::arg("keys"), py::arg("counts"), py::arg("rank"), py::arg("d_u"), py::arg("cap"),
        "launch_rank_scatter: the whole sorted keys / counts (cap entries, pattern where "
        "unwritten).");
  m.def("dict_scan_pack", [](const std::string& keys, const std::vector<u64>& counts,
                             u32 num_unique, u64 cap, u32 emit_limit, bool with_ctr_out,
                             const py::dict& ctr) {
    const std::vector<PackedKey> k = keys_from_blob(keys);
    DictStageCounters c = stage_counters_from(ctr);
    c.num_unique = num_unique;
    DictStageScanPack r;
    {
      py::gil_scoped_release nogil;
      r = dict_stage_scan_pack(k, counts, c, cap, emit_limit, with_ctr_out);
    }
    py::dict d;
    d["keys"] = blob_from_keys(r.records.data(), r.records.size());
    d["counts"] = counts_of(r.records);
    d["total_count"] = r.total_count;
    d["ctr_out"] = stage_counters_dict(r.ctr_out);
    d["tail_intact"] = r.tail_intact;
    d["untouched"] = r.untouched;
    return d;
  }, py::arg("keys"), py::arg("counts"), py::arg("num_unique"), py::arg("cap"),
        py::arg("emit_limit") = 0xFFFFFFFFu, py::arg("with_ctr_out") = true,
        py::arg("ctr") = py::dict(),
        "launch_scan_pack on zeroed look-back scratch: the records [0, num_unique), "
        "ctr.total_count (pattern bytes if unwritten), ctr_out, tail_intact, untouched.");
  m.def("part_plan", [](const std::vector<u64>& w0, const std::vector<u64>& counts, u32 d_u,
                        u32 ucap) {
    py::gil_scoped_release nogil;
    return dict_stage_part_plan(w0, counts, d_u, ucap);
  }, py::arg("w0"), py::arg("counts"), py::arg("d_u"), py::arg("ucap"),
        "launch_part_plan over first words and sample counts: the 257 range starts.");
  m.def("write_spill",
        [](const std::string& path, const std::vector<std::pair<std::string, u64>>& recs,
           const std::string& fmt) {
          std::vector<KeyCount> v;
          for (const auto& r : recs) {
            KeyCount kc{};
            PackedKey k = to_key(r.first);
            for (int w = 0; w < kKeyWords; ++w) kc.w[w] = k.w[w];
            kc.count = r.second;
            v.push_back(kc);
          }
          write_spill(path, v, fmt == "binary" ? SpillFormat::kBinary
                               : fmt == "kiv"  ? SpillFormat::kKiv
                                               : SpillFormat::kText);
        }, py::arg("path"), py::arg("recs"), py::arg("fmt") = "text");
  m.def("read_kiv", [](const std::string& path) {
    py::list out;
    for (const auto& r : read_kiv(path))
      out.append(py::make_tuple(py::bytes(key_to_string(r.key)), r.value, r.count));
    return out;
  }, py::arg("path"), "KeyIntValuePair records of a kiv file: (key, value, count).");
  m.def("read_spill", [](const std::string& path) {
    py::list out;
    for (const auto& r : read_spill(path)) {
      PackedKey k;
      for (int w = 0; w < kKeyWords; ++w) k.w[w] = r.w[w];
      out.append(py::make_tuple(py::bytes(key_to_string(k)), r.count));
    }
    return out;
  });
  m.def("find_line_window", [](const std::string& path, i64 s, i64 e) {
    py::gil_scoped_release nogil;
    const LineWindow w = find_line_window(path, s, e);
    return std::make_tuple(w.begin, w.end, w.lines);
  }, py::arg("path"), py::arg("line_start"), py::arg("line_end"),
        "(begin, end, lines) of the line window [line_start, line_end) of a file");
  m.def("byte_window", [](const std::string& path, u64 a, u64 b) {
    py::gil_scoped_release nogil;
    const LineWindow w = byte_window(path, a, b);
    return std::make_tuple(w.begin, w.end, w.lines);
  }, py::arg("path"), py::arg("begin"), py::arg("end"),
        "(begin, end, 0): bytes [begin, end) of a file moved to line starts");
  m.def("line_start_at", &line_start_at, py::arg("path"), py::arg("offset"));
  m.def("count_newlines", [](py::bytes b) {
    const std::string_view v = b;
    return count_newlines(v.data(), v.size());
  });
  m.def("count_lines", [](py::bytes b) {
    const std::string_view v = b;
    return count_lines(v.data(), v.size());
  });
  m.def("line_index_cache_path", &line_index_cache_path, py::arg("path"));
  m.def("native_stage", [] { return py::make_tuple(std::string(current_stage()), stages_entered()); },
        "(the distributed stage this process last entered, stages entered so far)");
  m.def("spill_index", [](const std::string& spill) -> py::object {
    SpillIndex x;
    if (!read_spill_index(spill, &x)) return py::none();
    py::dict d;
    d["sorted"] = x.sorted;
    d["distinct"] = x.distinct;
    d["records"] = x.records;
    d["total_count"] = x.total_count;
    d["spill_bytes"] = x.spill_bytes;
    d["stride"] = x.stride;
    py::list smp;
    for (const SpillSample& v : x.samples)
      smp.append(py::make_tuple(py::bytes(key_to_string(v.key)), v.record, v.offset, v.count_before));
    d["samples"] = smp;
    return d;
  }, py::arg("spill"), "The spill's sparse index (<spill>.idx), or None.");
  m.def("reducer_splitters", [](const std::vector<std::string>& spills, int reducers) {
    std::vector<SpillIndex> idx(spills.size());
    for (size_t k = 0; k < spills.size(); ++k) {
      if (!read_spill_index(spills[k], &idx[k])) {
        std::vector<KeyCount> v = read_spill(spills[k]);
        sort_combine(&v);
        idx[k] = index_records(v);
      }
    }
    py::list out;
    for (const PackedKey& k : plan_reducer_splitters(idx, reducers)) out.append(py::bytes(key_to_string(k)));
    return out;
  }, py::arg("spills"), py::arg("reducers"));
  m.def("reduce_spills", [](const JobConfig& cfg, const std::vector<std::string>& files, int reducer,
                           int reducers) {
    ReduceStageStats st;
    WordCountResult r;
    {
      py::gil_scoped_release nogil;
      r = reduce_spills(cfg, files, reducer, reducers, &st);
    }
    py::dict d;
    d["input_files"] = st.input_files;
    d["indexed_files"] = st.indexed_files;
    d["loaded_files"] = st.loaded_files;
    d["records_read"] = st.records_read;
    d["run_records"] = st.run_records;
    d["read_ms"] = st.read_ms;
    d["setup_ms"] = st.setup_ms;
    d["merge_ms"] = st.merge_ms;
    return py::make_tuple(PyResult{std::move(r)}, d);
  }, py::arg("cfg"), py::arg("files"), py::arg("reducer") = 0, py::arg("reducers") = 1,
        "Stage 2 over spill files: (result, stats); key range `reducer` of `reducers`.");
  m.def("map_stage", [](const JobConfig& cfg, const std::string& file, i64 s, i64 e,
                        const std::string& spill, const std::string& fmt) {
    MapStageResult r;
    {
      py::gil_scoped_release nogil;
      r = map_stage(cfg, file, s, e, spill,
                    fmt == "binary" ? SpillFormat::kBinary : fmt == "kiv" ? SpillFormat::kKiv
                                                                         : SpillFormat::kText);
    }
    py::dict d;
    d["lines"] = r.lines;
    d["tokens"] = r.result.num_tokens;
    d["unique"] = r.result.num_unique;
    d["spill_records"] = r.spill_records;
    d["spill_bytes"] = r.index.spill_bytes;
    d["input_bytes"] = r.input_bytes;
    d["streamed"] = r.streamed;
    d["map_ms"] = r.result.times.h2d_ms + r.result.times.map_ms;
    d["process_ms"] = r.result.times.process_ms + r.result.times.reduce_ms;
    d["job_ms"] = r.job_ms;
    return d;
  }, py::arg("cfg"), py::arg("file"), py::arg("line_start"), py::arg("line_end"),
        py::arg("spill"), py::arg("fmt") = "binary",
        "Stage 1 over a line window: the combined, indexed spill (see locust/stage.hpp).");
  m.def("partmap_cache_path", &partmap_cache_path, py::arg("input"), py::arg("cfg"));
  m.def("load_partmap_cache", [](const std::string& path) -> py::object {
    std::vector<u64> lo;
    if (!load_partmap_cache(path, &lo)) return py::none();
    return py::cast(lo);
  }, py::arg("path"));
  m.def("save_partmap_cache", &save_partmap_cache, py::arg("path"), py::arg("lo"));
  py::register_exception<Error>(m, "LocustError");
}
