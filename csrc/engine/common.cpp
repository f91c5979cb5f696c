// Shared host-side pieces: logging, errors, env config, tokenizer oracle, result checks.
#include <algorithm>
#include <map>
#include <atomic>
#include <chrono>
#include <malloc.h>

#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <string>
#include <thread>

#include "locust/config.hpp"
#include "locust/device/fuzzy.hpp"
#include "locust/device/glob.hpp"
#include "locust/device/regex.hpp"
#include "locust/dstring.hpp"
#include "locust/engine.hpp"

namespace locust {

int& log_rank() {
  static thread_local int r = -1;
  return r;
}

LogLevel log_level() {
  static LogLevel lvl = [] {
    const char* e = std::getenv("LOCUST_LOG");
    if (!e) return LogLevel::kWarn;
    std::string s(e);
    if (s == "error") return LogLevel::kError;
    if (s == "info") return LogLevel::kInfo;
    if (s == "debug") return LogLevel::kDebug;
    return LogLevel::kWarn;
  }();
  return lvl;
}

void log_msg(LogLevel lvl, const char* fmt, ...) {
  if ((int)lvl > (int)log_level()) return;
  static const char* names[] = {"ERROR", "WARN", "INFO", "DEBUG"};
  char buf[2048];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  // stderr only: stdout stays byte-compatible with the reference.
  if (log_rank() >= 0)
    std::fprintf(stderr, "[locust %s r%d] %s\n", names[(int)lvl], log_rank(), buf);
  else
    std::fprintf(stderr, "[locust %s] %s\n", names[(int)lvl], buf);
}

void throw_error(const char* file, int line, const std::string& msg) {
  std::string where = std::string(file) + ":" + std::to_string(line);
  std::string rank = log_rank() >= 0 ? ("rank " + std::to_string(log_rank()) + ": ") : "";
  throw Error(rank + msg + " (" + where + ")");
}

namespace {
std::atomic<const char*> g_stage{"none"};
std::atomic<u64> g_stages{0};
}  // namespace
void set_current_stage(const char* stage) {
  g_stage.store(stage, std::memory_order_relaxed);
  g_stages.fetch_add(1, std::memory_order_relaxed);
}
const char* current_stage() { return g_stage.load(std::memory_order_relaxed); }
u64 stages_entered() { return g_stages.load(std::memory_order_relaxed); }

bool fault_injected(int rank, const char* stage) {
  const char* e = std::getenv("LOCUST_FAULT");
  if (!e || !*e) return false;
  std::string s(e);
  auto colon = s.find(':');
  if (colon == std::string::npos) return false;
  int r = std::atoi(s.substr(0, colon).c_str());
  if (r != rank) return false;
  const std::string what = s.substr(colon + 1);
  if (what == std::string("hang_") + stage) {
    // a rank that stops answering (the SCALE watchdog's test, tests/test_scale_ready.py):
    // it never returns, like a peer stuck in a collective
    std::fprintf(stderr, "locust: rank %d: injected hang (LOCUST_FAULT) in stage '%s'\n", rank,
                 stage);
    std::fflush(stderr);
    for (;;) std::this_thread::sleep_for(std::chrono::seconds(1));
  }
  return what == stage;
}

namespace {
const u64 g_library_init_ns = now_ns();
}  // namespace
u64 library_init_ns() { return g_library_init_ns; }

u64 now_ns() {
  return (u64)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

u64 process_rss_kb(bool peak) {
  std::FILE* f = std::fopen("/proc/self/status", "r");
  if (!f) return 0;
  char line[256];
  unsigned long long kb = 0;
  const char* key = peak ? "VmHWM: %llu kB" : "VmRSS: %llu kB";
  while (std::fgets(line, sizeof(line), f))
    if (std::sscanf(line, key, &kb) == 1) break;
  std::fclose(f);
  return kb;
}

std::string process_rss_breakdown() {
  std::FILE* f = std::fopen("/proc/self/status", "r");
  if (!f) return "rss unknown";
  char line[256];
  unsigned long long rss = 0, hwm = 0, anon = 0, file = 0, shmem = 0, v = 0;
  while (std::fgets(line, sizeof(line), f)) {
    if (std::sscanf(line, "VmRSS: %llu kB", &v) == 1) rss = v;
    if (std::sscanf(line, "VmHWM: %llu kB", &v) == 1) hwm = v;
    if (std::sscanf(line, "RssAnon: %llu kB", &v) == 1) anon = v;
    if (std::sscanf(line, "RssFile: %llu kB", &v) == 1) file = v;
    if (std::sscanf(line, "RssShmem: %llu kB", &v) == 1) shmem = v;
  }
  std::fclose(f);
  // the heap's share of anon: bytes in use (arena + mmap'ed chunks) and the arenas' size
  const struct mallinfo2 mi = mallinfo2();
  char buf[256];
  std::snprintf(buf, sizeof(buf),
                "rss %llu kB (anon %llu, file %llu, shmem %llu; peak %llu; malloc in use %llu kB, "
                "arenas %llu kB, mmap'ed %llu kB)",
                rss, anon, file, shmem, hwm,
                (unsigned long long)((mi.uordblks + mi.hblkhd) >> 10),
                (unsigned long long)(mi.arena >> 10), (unsigned long long)(mi.hblkhd >> 10));
  return buf;
}

void apply_env_overrides(JobConfig& cfg) {
  if (const char* e = std::getenv("LOCUST_CHECK")) cfg.check = std::atoi(e) != 0;
  if (const char* e = std::getenv("LOCUST_REDUCE_PATH")) {
    std::string s(e);
    if (s == "lds") cfg.reduce_path = ReducePath::kLds;
    if (s == "global") cfg.reduce_path = ReducePath::kGlobal;
  }
  if (const char* e = std::getenv("LOCUST_MAP_PATH")) {
    std::string s(e);
    if (s == "compat") cfg.map_path = MapPath::kCompat;
    if (s == "fast") cfg.map_path = MapPath::kFast;
  }
  if (const char* e = std::getenv("LOCUST_SORT")) {
    std::string s(e);
    if (s == "radix") cfg.sort_path = SortPath::kRadix;
    if (s == "dict") cfg.sort_path = SortPath::kDict;
  }
  if (const char* e = std::getenv("LOCUST_CHUNK_MB")) cfg.chunk_bytes = (u64)std::atoll(e) << 20;
  if (const char* e = std::getenv("LOCUST_ZERO_COPY")) cfg.zero_copy_text = std::atoi(e);
  if (const char* e = std::getenv("LOCUST_GRAPH")) cfg.graph = std::atoi(e);
}

const char* to_string(ReducePath p) { return p == ReducePath::kLds ? "lds" : "global"; }
const char* to_string(MapPath p) { return p == MapPath::kCompat ? "compat" : "fast"; }
const char* to_string(SortPath p) { return p == SortPath::kRadix ? "radix" : "dict"; }

void check_ngram(const JobConfig& cfg) {
  if (cfg.ngram < 1 || cfg.ngram > kMaxNgram)
    throw Error("ngram must be in [1, " + std::to_string(kMaxNgram) + "], got " +
                std::to_string(cfg.ngram));
}

int tokenize_line(const char* line, u64 len, const JobConfig& cfg, std::vector<PackedKey>* out,
                  u64* truncated, std::vector<std::pair<u32, u32>>* at) {
  // The reference works on a NUL-terminated copy (main.cu:55-59); text after an embedded
  // NUL is invisible to strtok_r, exactly as here.
  std::string buf(line, len);
  char* save = nullptr;
  char* tok = d_strtok_r(&buf[0], cfg.delimiters.c_str(), &save);
  if (cfg.ngram > 1) {
    // Word n-grams: every token of the line (uncapped, untruncated), then the first
    // emits_per_line n-grams t_i ' ' ... ' ' t_(i+N-1); the key is the first max_key_len
    // bytes of the joined words.
    std::vector<std::pair<const char*, int>> toks;
    for (; tok != nullptr; tok = d_strtok_r(nullptr, cfg.delimiters.c_str(), &save))
      toks.emplace_back(tok, d_strlen(tok));
    const size_t N = (size_t)cfg.ngram;
    const size_t grams = toks.size() >= N ? toks.size() - N + 1 : 0;
    const size_t emit = std::min<size_t>(grams, (size_t)std::max(cfg.emits_per_line, 0));
    std::string joined;
    for (size_t i = 0; i < emit; ++i) {
      joined.assign(toks[i].first, (size_t)toks[i].second);
      for (size_t g = 1; g < N; ++g) {
        joined.push_back(' ');
        joined.append(toks[i + g].first, (size_t)toks[i + g].second);
      }
      int n = (int)std::min<size_t>(joined.size(), (size_t)cfg.max_key_len);
      if (joined.size() > (size_t)cfg.max_key_len && truncated) ++*truncated;
      PackedKey k;
      pack_key(joined.data(), n, k.w);
      out->push_back(k);
    }
    return grams > emit ? 1 : 0;
  }
  int count = 0;
  int dropped = 0;
  while (tok != nullptr) {
    if (count >= cfg.emits_per_line) {
      dropped = 1;
      break;
    }
    int n = d_strlen(tok);
    if (at) at->emplace_back((u32)(tok - buf.data()), (u32)n);
    if (n > cfg.max_key_len) {
      if (truncated) ++*truncated;
      n = cfg.max_key_len;
    }
    PackedKey k;
    pack_key(tok, n, k.w);
    out->push_back(k);
    ++count;
    tok = d_strtok_r(nullptr, cfg.delimiters.c_str(), &save);
  }
  return dropped;
}

void entries_from_sorted_tokens(const PackedKey* sorted, u64 n, std::vector<WordCountEntry>* out) {
  out->clear();
  u64 i = 0;
  while (i < n) {
    u64 j = i + 1;
    while (j < n && key_compare(sorted[j].w, sorted[i].w) == 0) ++j;
    out->push_back(WordCountEntry{sorted[i], j - i});
    i = j;
  }
}

// LOCUST_CHECK invariants: keys strictly increasing, no empty runs,
// counts sum to the token count.  (Runs are contiguous by construction: val is the
// prefix of the counts, EntryVals.)
void validate_result(const WordCountResult& r) {
  u64 sum = 0, j = 0;
  PackedKey prev{};
  for (const WordCountEntry e : r.entries) {  // compact lists decode on the fly
    if (j && key_compare(prev.w, e.key.w) >= 0)
      throw Error("LOCUST_CHECK: output keys not strictly increasing at entry " +
                  std::to_string(j));
    if (e.count == 0) throw Error("LOCUST_CHECK: zero count at entry " + std::to_string(j));
    sum += e.count;
    prev = e.key;
    ++j;
  }
  if (j != r.entries.size()) throw Error("LOCUST_CHECK: entry count mismatch");
  if (sum != r.num_tokens)
    throw Error("LOCUST_CHECK: sum(count)=" + std::to_string(sum) +
                " != num_tokens=" + std::to_string(r.num_tokens));
  if (r.entries.size() != r.num_unique) throw Error("LOCUST_CHECK: num_unique mismatch");
}

// ---- top-K by count: the host selection (engine.hpp) ----
namespace {
// rank order: count descending, then key ascending
bool top_before(const TopEntry& a, const TopEntry& b) {
  if (a.count != b.count) return a.count > b.count;
  return key_compare(a.key.w, b.key.w) < 0;
}
}  // namespace

std::vector<TopEntry> top_entries(const WordCountResult& r, u64 k) {
  std::vector<TopEntry> all;
  all.reserve(r.entries.size());
  EntryVals vals(r);
  for (const WordCountEntry e : r.entries) {  // either entry form
    const u64 val = vals.next(e);
    all.push_back(TopEntry{e.key, e.count, val});
  }
  const size_t m = (size_t)std::min<u64>(k, all.size());
  std::partial_sort(all.begin(), all.begin() + (std::ptrdiff_t)m, all.end(), top_before);
  all.resize(m);
  all.shrink_to_fit();
  return all;
}

TopResult top_result(const WordCountResult& r, u64 k) {
  TopResult t;
  t.entries = top_entries(r, k);
  t.k = k;
  t.num_lines = r.num_lines;
  t.num_tokens = r.num_tokens;
  t.num_unique = r.num_unique;
  t.overflow_lines = r.overflow_lines;
  t.truncated = r.truncated;
  t.max_key_len = r.max_key_len;
  t.chunks = r.chunks;
  t.times = r.times;
  return t;
}

void validate_top(const TopResult& t) {
  if (t.entries.size() != std::min<u64>(t.k, t.num_unique))
    throw Error("LOCUST_CHECK: top-k has " + std::to_string(t.entries.size()) +
                " entries, expected min(" + std::to_string(t.k) + ", " +
                std::to_string(t.num_unique) + ")");
  for (size_t j = 1; j < t.entries.size(); ++j) {
    const TopEntry &a = t.entries[j - 1], &b = t.entries[j];
    if (b.count > a.count)
      throw Error("LOCUST_CHECK: top-k counts increase at entry " + std::to_string(j));
    if (b.count == a.count && key_compare(a.key.w, b.key.w) >= 0)
      throw Error("LOCUST_CHECK: top-k tie not key-ascending at entry " + std::to_string(j));
  }
}

void format_top_output(const TopResult& t, bool cpu_format, std::string* out) {
  out->reserve(out->size() + t.entries.size() * 48);
  char buf[kKeyBytes + 1];
  for (const TopEntry& e : t.entries) {
    const int n = unpack_key(e.key.w, buf);
    if (n == 0) continue;
    out->append("print key: ");
    out->append(buf, (size_t)n);
    if (cpu_format) {
      out->append(" \t value: ");
      out->append(std::to_string(e.count));
    } else {
      out->append(" \t val: ");
      out->append(std::to_string(e.val));
      out->append(" \t count: ");
      out->append(std::to_string(e.count));
    }
    out->push_back('\n');
  }
}

// ---- corpus: the segment table (engine.hpp) ----
void IndexSegments::reset(u64 first, u64 lines) {
  segs.assign(1, IndexSegment{0, first, 0});
  first_line = first;
  num_lines = lines;
  next_id = 1;
}

void IndexSegments::append(u64 lines, bool new_file) {
  if (segs.empty()) reset(first_line, num_lines);
  if (new_file) {
    // (the host twins' refusal.  DevicePipeline::append_index makes the same check before it
    // enqueues anything, and that one is what keeps its index intact; the id check below cannot
    // fire there first: ids are u32 and at most kCorpusMaxFiles segments are resident.)
    LOCUST_CHECK_ARG(segs.size() < kCorpusMaxFiles,
                     "append_index: the index holds " + std::to_string(segs.size()) +
                         " files, the most it takes (kCorpusMaxFiles = " +
                         std::to_string(kCorpusMaxFiles) + "): drop the oldest first");
    LOCUST_CHECK_ARG(next_id != 0xffffffffu, "append_index: file ids past 2^32 - 1");
    segs.push_back(IndexSegment{next_id++, first_line + num_lines, 0});
  }
  num_lines += lines;
}

u64 IndexSegments::drop(u64 lines) {
  if (segs.empty()) reset(first_line, num_lines);
  LOCUST_CHECK_ARG(lines <= num_lines, "drop_index: " + std::to_string(lines) +
                                           " lines to drop, the index holds " +
                                           std::to_string(num_lines));
  if (lines == 0) return 0;
  const u64 cut = first_line + lines;
  size_t k = 0;  // the last segment that begins at or before the cut: the first to stay
  while (k + 1 < segs.size() && segs[k + 1].first_line <= cut) ++k;
  u64 gone = 0;
  for (size_t i = 0; i < k; ++i) gone += lines_of(i) != 0;
  segs.erase(segs.begin(), segs.begin() + (std::ptrdiff_t)k);
  segs[0].base += cut - segs[0].first_line;
  segs[0].first_line = cut;
  first_line = cut;
  num_lines -= lines;
  return gone;
}

size_t IndexSegments::locate(u64 line) const {
  LOCUST_CHECK_ARG(!segs.empty() && line >= first_line && line < first_line + num_lines,
                   "locate: line " + std::to_string(line) + " outside the resident lines [" +
                       std::to_string(first_line) + ", " + std::to_string(first_line + num_lines) +
                       ")");
  // the last segment with first_line <= line
  const auto it = std::upper_bound(segs.begin(), segs.end(), line,
                                   [](u64 l, const IndexSegment& s) { return l < s.first_line; });
  return (size_t)(it - segs.begin()) - 1;
}

size_t IndexSegments::find(u32 id) const {
  const auto it = std::lower_bound(segs.begin(), segs.end(), id,
                                   [](const IndexSegment& s, u32 i) { return s.id < i; });
  return it != segs.end() && it->id == id ? (size_t)(it - segs.begin()) : segs.size();
}

IndexSegments IndexResult::segment_table() const {
  IndexSegments t;
  t.reset(first_line, words.num_lines);
  if (!segments.empty()) {
    t.segs = segments;
    t.next_id = segments.back().id + 1;
  }
  return t;
}

// ---- inverted index (engine.hpp) ----
void validate_index(const IndexResult& r) {
  validate_result(r.words);
  if (r.postings.size() != r.words.num_tokens)
    throw Error("LOCUST_CHECK: index has " + std::to_string(r.postings.size()) +
                " postings, num_tokens=" + std::to_string(r.words.num_tokens));
  const u64 lo = r.first_line, hi = r.first_line + r.words.num_lines;
  for (size_t i = 0; i < r.segments.size(); ++i) {
    const IndexSegment& sg = r.segments[i];
    if ((i == 0 ? sg.first_line != lo : sg.first_line < r.segments[i - 1].first_line ||
                                            sg.id <= r.segments[i - 1].id) ||
        sg.first_line > hi || (i && sg.base))
      throw Error("LOCUST_CHECK: segment " + std::to_string(i) + " (id " + std::to_string(sg.id) +
                  ", first line " + std::to_string(sg.first_line) + ", base " +
                  std::to_string(sg.base) + ") does not continue the table over [" +
                  std::to_string(lo) + ", " + std::to_string(hi) + ")");
  }
  u64 at = 0, j = 0;
  for (const WordCountEntry e : r.words.entries) {
    for (u64 k = 0; k < e.count; ++k) {
      const u64 l = r.postings[at + k];
      if (l < lo || l >= hi)
        throw Error("LOCUST_CHECK: posting " + std::to_string(l) + " of entry " +
                    std::to_string(j) + " outside the lines [" + std::to_string(lo) + ", " +
                    std::to_string(hi) + ")");
      if (k && l < r.postings[at + k - 1])
        throw Error("LOCUST_CHECK: postings of entry " + std::to_string(j) +
                    " decrease at position " + std::to_string(k));
    }
    at += e.count;
    ++j;
  }
}

void format_index_output(const IndexResult& r, std::string* out) {
  out->reserve(out->size() + r.words.entries.size() * 40 + r.postings.size() * 6);
  char buf[kKeyBytes + 1];
  u64 at = 0;
  for (const WordCountEntry e : r.words.entries) {  // either entry form
    const int n = unpack_key(e.key.w, buf);
    const u64 from = at;
    at += e.count;
    if (n == 0) continue;
    out->append("print key: ");
    out->append(buf, (size_t)n);
    out->append(" \t count: ");
    out->append(std::to_string(e.count));
    out->append(" \t lines:");
    for (u64 k = from; k < at && k < r.postings.size(); ++k) {
      out->push_back(' ');
      out->append(std::to_string(r.postings[k]));
    }
    out->push_back('\n');
  }
}

// ---- appending to the index: the host twin of kernels/append.hip (engine.hpp) ----
IndexResult merge_index(const IndexResult& a, const IndexResult& b, bool new_file) {
  LOCUST_CHECK_ARG(b.first_line == a.first_line + a.words.num_lines,
                   "merge_index: the second index starts at line " + std::to_string(b.first_line) +
                       ", the first one ends before line " +
                       std::to_string(a.first_line + a.words.num_lines));
  LOCUST_CHECK_ARG(b.first_line + b.words.num_lines <= (1ull << 32),
                   "index: line numbers past 2^32 do not fit a u32 posting");
  IndexResult c;
  c.first_line = a.first_line;
  {
    IndexSegments t = a.segment_table();
    t.append(b.words.num_lines, new_file);
    c.segments = std::move(t.segs);
  }
  WordCountResult& w = c.words;
  w.num_lines = a.words.num_lines + b.words.num_lines;
  w.num_tokens = a.words.num_tokens + b.words.num_tokens;
  w.overflow_lines = a.words.overflow_lines + b.words.overflow_lines;
  w.truncated = a.words.truncated + b.words.truncated;
  w.max_key_len = std::max(a.words.max_key_len, b.words.max_key_len);
  std::vector<WordCountEntry> e;
  e.reserve(a.words.entries.size() + b.words.entries.size());
  c.postings.reserve(a.postings.size() + b.postings.size());
  auto ia = a.words.entries.begin(), ib = b.words.entries.begin();
  const auto ea = a.words.entries.end(), eb = b.words.entries.end();
  u64 at_a = 0, at_b = 0, misplaced = 0;
  const auto take = [&](const IndexResult& x, u64* at, u64 count) {
    if (*at + count > x.postings.size())
      throw Error("merge_index: the counts of an index exceed its " +
                  std::to_string(x.postings.size()) + " postings");
    c.postings.insert(c.postings.end(), x.postings.begin() + (std::ptrdiff_t)*at,
                      x.postings.begin() + (std::ptrdiff_t)(*at + count));
    *at += count;
  };
  while (ia != ea || ib != eb) {
    const int cmp = ia == ea ? 1 : ib == eb ? -1 : key_compare((*ia).key.w, (*ib).key.w);
    WordCountEntry x = cmp <= 0 ? *ia : *ib;
    if (!e.empty() && key_compare(e.back().key.w, x.key.w) >= 0) ++misplaced;  // key order
    if (cmp <= 0) {
      take(a, &at_a, x.count);
      ++ia;
    }
    if (cmp >= 0) {
      const u64 cb = (*ib).count;
      take(b, &at_b, cb);
      if (cmp == 0) x.count += cb;
      ++ib;
    }
    e.push_back(x);
  }
  if (misplaced)
    throw Error("merge_index: " + std::to_string(misplaced) +
                " keys out of order: both indexes must hold their words in key order");
  if (at_a != a.postings.size() || at_b != b.postings.size() ||
      c.postings.size() != w.num_tokens)
    throw Error("merge_index: " + std::to_string(c.postings.size()) + " postings moved, " +
                std::to_string(w.num_tokens) + " tokens in the two indexes");
  LOCUST_CHECK_ARG(e.size() < (1ull << 32) && w.num_tokens < (1ull << 32),
                   "index: " + std::to_string(e.size()) + " words / " +
                       std::to_string(w.num_tokens) +
                       " tokens do not fit the 32-bit halves of a pair word");
  w.entries = std::move(e);
  w.num_unique = w.entries.size();
  return c;
}

// ---- dropping the oldest lines: the host twin of kernels/drop.hip (engine.hpp) ----
IndexResult trim_index(const IndexResult& x, u64 lines, u64 dropped_overflow_lines,
                       u64 dropped_truncated) {
  LOCUST_CHECK_ARG(lines <= x.words.num_lines,
                   "trim_index: " + std::to_string(lines) + " lines to drop, the index holds " +
                       std::to_string(x.words.num_lines));
  LOCUST_CHECK_ARG(dropped_overflow_lines <= x.words.overflow_lines &&
                       dropped_truncated <= x.words.truncated,
                   "trim_index: the dropped lines' statistics (" +
                       std::to_string(dropped_overflow_lines) + " lines over the emit cap, " +
                       std::to_string(dropped_truncated) + " truncated tokens) exceed the index's (" +
                       std::to_string(x.words.overflow_lines) + ", " +
                       std::to_string(x.words.truncated) + ")");
  const u64 cut = x.first_line + lines;
  IndexResult c;
  c.first_line = cut;
  {
    IndexSegments t = x.segment_table();
    t.drop(lines);
    c.segments = std::move(t.segs);
  }
  WordCountResult& w = c.words;
  w.num_lines = x.words.num_lines - lines;
  w.overflow_lines = x.words.overflow_lines - dropped_overflow_lines;
  w.truncated = x.words.truncated - dropped_truncated;
  w.max_key_len = x.words.max_key_len;  // (a maximum: the longest the index has held)
  w.times = x.words.times;
  std::vector<WordCountEntry> e;
  e.reserve(x.words.entries.size());
  c.postings.reserve(x.postings.size());
  u64 at = 0, misplaced = 0, dropped = 0;
  PackedKey prev{};
  bool have_prev = false;
  for (const WordCountEntry r : x.words.entries) {  // either entry form
    if (at + r.count > x.postings.size())
      throw Error("trim_index: the counts of the index exceed its " +
                  std::to_string(x.postings.size()) + " postings");
    if (have_prev && key_compare(prev.w, r.key.w) >= 0) ++misplaced;  // key order
    prev = r.key;
    have_prev = true;
    const auto first = x.postings.begin() + (std::ptrdiff_t)at;
    const auto last = first + (std::ptrdiff_t)r.count;
    if (!std::is_sorted(first, last)) ++misplaced;  // a list that decreases
    const auto keep = std::lower_bound(first, last, cut,
                                       [](u32 l, u64 line) { return (u64)l < line; });
    dropped += (u64)(keep - first);
    if (keep != last) {
      WordCountEntry k = r;
      k.count = (u64)(last - keep);
      e.push_back(k);
      c.postings.insert(c.postings.end(), keep, last);
    }
    at += r.count;
  }
  if (misplaced)
    throw Error("trim_index: " + std::to_string(misplaced) +
                " keys or postings out of order: the index must hold its words in key order and "
                "every list ascending");
  if (at != x.postings.size() || c.postings.size() + dropped != x.words.num_tokens)
    throw Error("trim_index: " + std::to_string(c.postings.size()) + " postings moved and " +
                std::to_string(dropped) + " dropped, " + std::to_string(x.words.num_tokens) +
                " tokens in the index");
  w.num_tokens = c.postings.size();
  w.entries = std::move(e);
  w.num_unique = w.entries.size();
  return c;
}

std::vector<TextInput> split_blocks(const TextInput& in, u64 block_bytes) {
  LOCUST_CHECK_ARG(block_bytes > 0, "split_blocks: block_bytes must be > 0 (--block-kb N, N >= 1)");
  LOCUST_CHECK_ARG(!in.source, "split_blocks takes a text held in memory, not a source");
  std::vector<TextInput> out;
  const char* p = in.data;
  const char* end = in.data + in.bytes;
  u64 line = in.first_line;
  while (p < end) {
    TextInput b;
    b.data = p;
    b.first_line = line;
    while (p < end) {  // whole lines while they fit
      const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
      const char* next = nl ? nl + 1 : end;
      if ((u64)(next - b.data) > block_bytes) {
        if (p == b.data)
          throw Error("line " + std::to_string(line) + " holds " + std::to_string(next - p) +
                      " bytes, more than a block of " + std::to_string(block_bytes) +
                      " bytes: a block is whole lines (raise --block-kb)");
        break;
      }
      p = next;
      ++line;
    }
    b.bytes = (u64)(p - b.data);
    b.num_lines = line - b.first_line;
    out.push_back(b);
  }
  if (out.empty()) {  // an empty text is one empty block
    TextInput b;
    b.data = in.data;
    b.first_line = in.first_line;
    out.push_back(b);
  }
  return out;
}

// ---- index search: the host evaluation (engine.hpp) ----
PackedKey search_term_key(const std::string& term, const JobConfig& cfg) {
  PackedKey k;
  pack_key(term.data(), (int)std::min<size_t>(term.size(), (size_t)cfg.max_key_len), k.w);
  return k;
}

// ---- regex terms (engine.hpp): source -> the Glushkov position automaton ----
namespace {

// Recursive descent: alt := concat (`|` concat)*; concat := repeat*; repeat := atom [*+?];
// atom := literal | `.` | class | `(` alt `)`.  Every atom but a group is a new position; a
// fragment is the (first, last, nullable) of what it has read, and follow grows as fragments
// are joined.  The recursion is one level per open parenthesis, at most kRegexMaxDepth.
struct RegexCompiler {
  const std::string& src;
  bool fold;
  std::vector<u32>& prog;
  size_t at = 0;
  u32 npos = 0;

  struct Frag {
    u32 first = 0, last = 0;
    bool nullable = true;
  };

  [[noreturn]] void refuse(const std::string& why) const {
    std::string shown;  // (a NUL would end the message, a newline break it)
    for (const char ch : src) shown += ch == '\0' ? "\\0" : ch == '\n' ? "\\n" : std::string(1, ch);
    throw Error("search: the regex /" + shown + "/ " + why);
  }
  bool done() const { return at == src.size(); }

  // the byte behind a backslash (at: the backslash)
  unsigned char escaped() {
    if (at + 1 >= src.size()) refuse("ends in a backslash that escapes nothing");
    const unsigned char c = (unsigned char)src[at + 1];
    if ((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))
      refuse(std::string("holds \\") + (char)c +
             ": a backslash before a letter or digit is reserved (there is no \\d or \\w)");
    at += 2;
    return c;
  }

  // a new position that accepts `set` (taken before a class's negation)
  Frag position(bool (&set)[256], bool negate) {
    if (npos == (u32)kRegexMaxPos)
      refuse("has more than kRegexMaxPos = " + std::to_string(kRegexMaxPos) +
             " positions (literals, dots and classes)");
    if (fold)
      for (int c = 'a'; c <= 'z'; ++c) set[c] = set[c ^ 0x20] = set[c] || set[c ^ 0x20];
    const u32 bit = 1u << npos++;
    for (int c = 1; c < 256; ++c)  // (B[0] stays 0: nothing accepts the padding)
      if (set[c] != negate) prog[(size_t)(kRegexB + c)] |= bit;
    Frag f;
    f.first = f.last = bit;
    f.nullable = false;
    return f;
  }

  Frag parse_class() {  // (at: behind the `[`)
    bool set[256] = {};
    bool negate = false, any = false;
    if (!done() && src[at] == '^') {
      negate = true;
      ++at;
    }
    for (;;) {
      if (done()) refuse("holds an unterminated class: a [ without its ]");
      if (src[at] == ']') {
        ++at;
        break;
      }
      unsigned char lo;
      if (src[at] == '\\') {
        lo = escaped();
      } else {
        lo = (unsigned char)src[at++];
      }
      unsigned char hi = lo;
      // a range: a `-` that is not the class's last byte
      if (at + 1 < src.size() && src[at] == '-' && src[at + 1] != ']') {
        ++at;
        if (src[at] == '\\') {
          hi = escaped();
        } else {
          hi = (unsigned char)src[at++];
        }
        if (lo > hi)
          refuse(std::string("holds the range ") + (char)lo + "-" + (char)hi +
                 ", whose first byte lies behind its last (lo > hi)");
      }
      for (int c = lo; c <= hi; ++c) set[c] = true;
      any = true;
    }
    if (!any) refuse("holds an empty class: [] and [^] have no member (escape a ] as \\])");
    return position(set, negate);
  }

  Frag parse_atom(int depth) {
    const char ch = src[at];
    if (ch == '(') {
      if (depth >= kRegexMaxDepth)
        refuse("nests parentheses deeper than kRegexMaxDepth = " + std::to_string(kRegexMaxDepth));
      ++at;
      const Frag f = parse_alt(depth + 1);
      if (done() || src[at] != ')') refuse("has unbalanced parentheses: a ( is never closed");
      ++at;
      return f;
    }
    bool set[256] = {};
    if (ch == '[') {
      ++at;
      return parse_class();
    }
    if (ch == '.') {
      ++at;
      for (int c = 1; c < 256; ++c) set[c] = true;
      return position(set, false);
    }
    if (ch == '{' || ch == '}' || ch == '^' || ch == '$')
      refuse(std::string("holds an unescaped ") + ch +
             " outside a class: counted repeats and anchors are not supported (a term is "
             "anchored at both ends already); write \\" + ch + " for the byte");
    if (ch == '\\') {
      set[escaped()] = true;
    } else {
      set[(unsigned char)ch] = true;
      ++at;
    }
    return position(set, false);
  }

  Frag parse_repeat(int depth) {
    const char ch = src[at];
    if (ch == '*' || ch == '+' || ch == '?')
      refuse(std::string("holds a quantifier ") + ch + " with nothing to repeat");
    Frag f = parse_atom(depth);
    if (done()) return f;
    const char qc = src[at];
    if (qc != '*' && qc != '+' && qc != '?') return f;
    ++at;
    if (qc != '?')
      for (u32 i = 0; i < npos; ++i)
        if ((f.last >> i) & 1u) prog[(size_t)(kRegexFollow + (int)i)] |= f.first;
    if (qc != '+') f.nullable = true;
    if (!done() && (src[at] == '*' || src[at] == '+' || src[at] == '?'))
      refuse(std::string("holds the quantifier ") + src[at] + " directly after the quantifier " +
             qc + ": lazy and stacked quantifiers are not supported");
    return f;
  }

  Frag parse_concat(int depth) {
    Frag r;  // the empty string
    while (!done() && src[at] != '|' && src[at] != ')') {
      const Frag f = parse_repeat(depth);
      for (u32 i = 0; i < npos; ++i)
        if ((r.last >> i) & 1u) prog[(size_t)(kRegexFollow + (int)i)] |= f.first;
      const Frag a = r;
      r.first = a.first | (a.nullable ? f.first : 0u);
      r.last = f.last | (f.nullable ? a.last : 0u);
      r.nullable = a.nullable && f.nullable;
    }
    return r;
  }

  Frag parse_alt(int depth) {
    Frag r = parse_concat(depth);
    while (!done() && src[at] == '|') {
      ++at;
      const Frag f = parse_concat(depth);
      r.first |= f.first;
      r.last |= f.last;
      r.nullable = r.nullable || f.nullable;
    }
    return r;
  }
};

}  // namespace

std::vector<u32> compile_regex(const std::string& source, bool ignore_case) {
  std::vector<u32> prog((size_t)kRegexWords, 0u);
  RegexCompiler c{source, ignore_case, prog};
  if (source.empty()) c.refuse("has an empty source: give an expression between the slashes");
  if (source.size() > kRegexMaxSource)
    c.refuse("has a source of " + std::to_string(source.size()) +
             " bytes; a source takes at most kRegexMaxSource = " +
             std::to_string(kRegexMaxSource));
  for (const char ch : source)
    if (ch == '\0' || ch == '\n')
      c.refuse("holds a NUL or a newline, which no word can hold");
  const RegexCompiler::Frag f = c.parse_alt(0);
  if (!c.done()) c.refuse("has unbalanced parentheses: a ) closes nothing");
  prog[kRegexFirst] = f.first;
  prog[kRegexLast] = f.last;
  prog[kRegexNullable] = f.nullable ? 1u : 0u;
  prog[kRegexNpos] = c.npos;
  return prog;
}

bool SearchPattern::matches(const u64* key, bool fold) const {
  if (regex) return regex_match(rx.data(), key);  // (the fold: compiled in)
  if (budget)
    return fuzzy_match(p.w[0], p.w[1], p.w[2], p.w[3], budget, key[0], key[1], key[2], key[3],
                       fold);
  return glob_match(p.w, meta, key, fold);
}

SearchQuery make_search_query(const std::vector<std::string>& terms, SearchMode mode,
                              bool wildcard, u64 within, const std::vector<std::string>& exclude,
                              bool glob, bool fuzzy, bool regex) {
  SearchQuery q;
  q.terms = terms;
  q.terms.insert(q.terms.end(), exclude.begin(), exclude.end());
  q.excluded = (u32)exclude.size();
  q.mode = mode;
  q.within = within;
  // the regex reading comes before every other: /source/, and nothing inside it is read again
  std::vector<u8> fz(q.terms.size(), 0);  // (a regex term: 0xff, so the readings below skip it)
  if (regex) {
    std::vector<u8> rx(q.terms.size(), 0);
    bool any_regex = false;
    for (size_t t = 0; t < q.terms.size(); ++t) {
      std::string& s = q.terms[t];
      if (s.empty() || s[0] != '/') continue;
      size_t slashes = 0;  // the backslashes before the last byte
      while (s.size() >= 3 && slashes < s.size() - 2 && s[s.size() - 2 - slashes] == '\\') ++slashes;
      LOCUST_CHECK_ARG(s.size() >= 3 && s.back() == '/' && slashes % 2 == 0,
                       "search: the term " + s + " starts with / but is no regex term: a regex "
                       "term is /source/, at least three bytes that end in a / that is not "
                       "escaped");
      s = s.substr(1, s.size() - 2);
      (void)compile_regex(s, false);  // (throws with the cause)
      rx[t] = 1;
      fz[t] = 0xff;
      any_regex = true;
    }
    if (any_regex) q.regex = std::move(rx);
  }
  // the fuzzy reading comes next: a trailing ~d, and the word before it
  if (fuzzy) {
    bool any_fuzzy = false;
    for (size_t t = 0; t < q.terms.size(); ++t) {
      if (fz[t]) continue;  // a regex term
      std::string& s = q.terms[t];
      if (s.size() < 3 || s[s.size() - 2] != '~' || s.back() < '0' || s.back() > '9') continue;
      const u32 d = (u32)(s.back() - '0');
      LOCUST_CHECK_ARG(d >= 1 && d <= kFuzzyMaxBudget,
                       "search: the fuzzy term " + s + " asks for a budget of " +
                           std::to_string(d) + " edits; a budget is 1 or 2 (word~1, word~2)");
      s.resize(s.size() - 2);
      LOCUST_CHECK_ARG(s.size() > (size_t)d,
                       "search: the fuzzy term " + s + "~" + std::to_string(d) + " has a word of " +
                           std::to_string(s.size()) + " bytes; a fuzzy term's word is longer than "
                           "its budget (it would match every word of up to " +
                           std::to_string(s.size() + d) + " bytes)");
      LOCUST_CHECK_ARG(!(glob || wildcard) || s.find_first_of("*?") == std::string::npos,
                       "search: the fuzzy term " + s + "~" + std::to_string(d) + " holds a * or a "
                       "? while wildcard or glob is on; a term is fuzzy or a pattern, never both");
      fz[t] = (u8)d;
      any_fuzzy = true;
    }
    if (any_fuzzy) {
      q.fuzzy = fz;
      for (u8& d : q.fuzzy)
        if (d == 0xff) d = 0;
    }
  }
  if (glob) {
    bool any_prefix = false, any_pattern = false;
    std::vector<u8> prefix(q.terms.size(), 0), pattern(q.terms.size(), 0);
    for (size_t t = 0; t < q.terms.size(); ++t) {
      if (fz[t]) continue;  // a fuzzy term: its word is literal
      std::string& s = q.terms[t];
      std::string c;  // runs of stars collapsed
      for (const char ch : s)
        if (ch != '*' || c.empty() || c.back() != '*') c.push_back(ch);
      LOCUST_CHECK_ARG(c != "*", "search: a pattern of stars alone is no term: give at least "
                                 "one other byte (ham*, *ing, h?mlet)");
      const size_t meta = c.find_first_of("*?");
      if (meta == std::string::npos) continue;  // a plain term (s == c: it holds no star)
      s = c;
      if (meta == s.size() - 1 && s.back() == '*') {  // p*: the prefix term
        s.pop_back();
        prefix[t] = 1;
        any_prefix = true;
      } else {
        pattern[t] = 1;
        any_pattern = true;
      }
    }
    if (any_prefix) q.prefix = std::move(prefix);
    if (any_pattern) q.pattern = std::move(pattern);
    return q;
  }
  if (!wildcard) return q;
  bool any = false;
  std::vector<u8> prefix(q.terms.size(), 0);
  for (size_t t = 0; t < q.terms.size(); ++t) {
    if (fz[t]) continue;  // a fuzzy term: its word is literal
    std::string& s = q.terms[t];
    LOCUST_CHECK_ARG(s != "*", "search: a lone * is no prefix term: give the prefix before "
                               "the star (ham*)");
    if (s.size() > 1 && s.back() == '*') {
      s.pop_back();
      prefix[t] = 1;
      any = true;
    }
  }
  if (any) q.prefix = std::move(prefix);
  return q;
}

// ---- boolean expressions (engine.hpp): tokens -> terms and a 256-bit truth table ----
namespace {

using Truth = std::array<u32, kExprTruthWords>;

// The table of the variable t: bit m set when mask m holds term t.
Truth truth_of_term(u32 t) {
  static const u32 kLow[5] = {0xaaaaaaaau, 0xccccccccu, 0xf0f0f0f0u, 0xff00ff00u, 0xffff0000u};
  Truth r{};
  for (u32 w = 0; w < (u32)kExprTruthWords; ++w)
    r[w] = t < 5 ? kLow[t] : (((w >> (t - 5)) & 1u) ? ~0u : 0u);
  return r;
}

// Recursive descent over the tokens: or := and (OR and)*; and := not ((AND)? not)*;
// not := NOT* atom; atom := term | ( or ).  The recursion is one level per open parenthesis,
// at most kExprMaxDepth; a run of NOT is a loop.
struct ExprParser {
  const std::vector<std::string>& tok;
  bool wildcard, glob, fuzzy, regex;
  SearchQuery* q;
  std::vector<u8> prefix, pattern, fz, rx;
  size_t at = 0;

  static bool is_op(const std::string& s) { return s == "AND" || s == "OR" || s == "NOT"; }
  bool done() const { return at == tok.size(); }
  // does an operand start here?
  bool operand_ahead() const {
    return !done() && tok[at] != ")" && tok[at] != "AND" && tok[at] != "OR";
  }

  u32 term_number(const std::string& asked) {
    const SearchQuery one =
        make_search_query({asked}, SearchMode::kAll, wildcard, 0, {}, glob, fuzzy, regex);
    const u8 pre = one.is_prefix(0) ? 1 : 0, pat = one.is_pattern(0) ? 1 : 0;
    const u8 bud = (u8)one.fuzzy_budget(0), re = one.is_regex(0) ? 1 : 0;
    for (size_t t = 0; t < q->terms.size(); ++t)
      if (q->terms[t] == one.terms[0] && prefix[t] == pre && pattern[t] == pat && fz[t] == bud &&
          rx[t] == re)
        return (u32)t;
    LOCUST_CHECK_ARG(q->terms.size() < (size_t)kSearchMaxTerms,
                     "search: the expression has more than " + std::to_string(kSearchMaxTerms) +
                         " distinct terms (" + asked + " is one too many)");
    q->terms.push_back(one.terms[0]);
    prefix.push_back(pre);
    pattern.push_back(pat);
    fz.push_back(bud);
    rx.push_back(re);
    return (u32)q->terms.size() - 1;
  }

  Truth parse_atom(int depth) {
    bool neg = false;
    while (!done() && tok[at] == "NOT") {
      neg = !neg;
      ++at;
    }
    LOCUST_CHECK_ARG(!done(), "search: the expression ends behind a dangling operator (" +
                                  (at ? tok[at - 1] : std::string("nothing")) +
                                  "): an operand is missing");
    const std::string& s = tok[at];
    LOCUST_CHECK_ARG(s != "AND" && s != "OR",
                     "search: a dangling operator: " + s + " stands where an operand belongs");
    LOCUST_CHECK_ARG(s != ")", at && tok[at - 1] == "("
                                   ? std::string("search: () holds no operand")
                                   : std::string("search: a dangling operator: ) stands where an "
                                                 "operand belongs"));
    Truth r;
    if (s == "(") {
      LOCUST_CHECK_ARG(depth < kExprMaxDepth,
                       "search: the expression nests parentheses deeper than kExprMaxDepth = " +
                           std::to_string(kExprMaxDepth));
      ++at;
      LOCUST_CHECK_ARG(done() || tok[at] != ")", "search: () holds no operand");
      r = parse_or(depth + 1);
      LOCUST_CHECK_ARG(!done() && tok[at] == ")",
                       "search: unbalanced parentheses: a ( is never closed");
      ++at;
    } else {
      r = truth_of_term(term_number(s));
      ++at;
    }
    if (neg)
      for (u32& w : r) w = ~w;
    return r;
  }
  Truth parse_and(int depth) {
    Truth r = parse_atom(depth);
    for (;;) {
      if (!done() && tok[at] == "AND")
        ++at;
      else if (!operand_ahead())
        return r;
      const Truth o = parse_atom(depth);
      for (int w = 0; w < kExprTruthWords; ++w) r[w] &= o[w];
    }
  }
  Truth parse_or(int depth) {
    Truth r = parse_and(depth);
    while (!done() && tok[at] == "OR") {
      ++at;
      const Truth o = parse_and(depth);
      for (int w = 0; w < kExprTruthWords; ++w) r[w] |= o[w];
    }
    return r;
  }
};

}  // namespace

SearchQuery make_search_expr(const std::string& expr, const JobConfig& cfg, bool wildcard,
                             bool glob, bool fuzzy, bool regex) {
  std::vector<std::string> tok;
  std::string cur;
  const auto flush = [&] {
    if (!cur.empty()) tok.push_back(cur);
    cur.clear();
  };
  // as asked: runs of blanks collapsed to one space, the ends trimmed (a regex token's bytes kept)
  std::string asked;
  bool gap = false;
  const auto keep = [&](char ch) {
    if (gap) asked.push_back(' ');
    gap = false;
    asked.push_back(ch);
  };
  for (size_t i = 0; i < expr.size(); ++i) {
    const char ch = expr[i];
    if (regex && ch == '/' && cur.empty()) {
      // "regex terms": a token that begins with / runs to the next unescaped /, blanks and
      // parentheses included
      size_t j = i + 1;
      while (j < expr.size() && expr[j] != '/') j += expr[j] == '\\' ? 2 : 1;
      LOCUST_CHECK_ARG(j < expr.size(), "search: the regex term that starts at byte " +
                                            std::to_string(i) + " of the expression has no "
                                            "closing /");
      LOCUST_CHECK_ARG(j + 1 == expr.size() || expr[j + 1] == ' ' || expr[j + 1] == '\t' ||
                           expr[j + 1] == '(' || expr[j + 1] == ')',
                       "search: the regex term " + expr.substr(i, j + 1 - i) + " is followed by "
                       "the byte " + std::string(1, expr[j + 1 < expr.size() ? j + 1 : j]) +
                           "; its closing / must be followed by a blank, a parenthesis or the end");
      for (size_t k = i; k <= j; ++k) keep(expr[k]);
      tok.push_back(expr.substr(i, j + 1 - i));
      i = j;
      continue;
    }
    if (ch == ' ' || ch == '\t') {
      flush();
      gap = !asked.empty();
      continue;
    }
    keep(ch);
    if (ch == '(' || ch == ')') {
      flush();
      tok.emplace_back(1, ch);
    } else {
      cur.push_back(ch);
    }
  }
  flush();
  LOCUST_CHECK_ARG(!tok.empty(), "search: an empty expression");
  SearchQuery q;
  q.mode = SearchMode::kExpr;
  q.expr = asked;
  ExprParser p{tok, wildcard, glob, fuzzy, regex, &q, {}, {}, {}, {}, 0};
  q.truth = p.parse_or(0);
  LOCUST_CHECK_ARG(p.done(), p.tok[p.at] == ")"
                                 ? std::string("search: unbalanced parentheses: a ) closes nothing")
                                 : "search: a dangling operator: " + p.tok[p.at] +
                                       " stands where the expression should end");
  // (only the masks over the query's own terms matter: the others repeat them)
  for (const u8 f : p.prefix)
    if (f) q.prefix = p.prefix;
  for (const u8 f : p.pattern)
    if (f) q.pattern = p.pattern;
  for (const u8 f : p.fz)
    if (f) q.fuzzy = p.fz;
  for (const u8 f : p.rx)
    if (f) q.regex = p.rx;
  check_search_queries({q}, cfg);
  return q;
}

void check_search_queries(const std::vector<SearchQuery>& queries, const JobConfig& cfg) {
  for (size_t i = 0; i < queries.size(); ++i) {
    const SearchQuery& q = queries[i];
    if (q.mode == SearchMode::kExpr) {
      LOCUST_CHECK_ARG(q.excluded == 0 && q.within == 0,
                       "search: query " + std::to_string(i) + " is an expression: it takes no "
                       "exclusion terms (exclude, --not) and no window (within): write NOT in the "
                       "expression instead");
      LOCUST_CHECK_ARG(!q.expr.empty(), "search: query " + std::to_string(i) +
                                            " is an expression query without an expression (use "
                                            "make_search_expr)");
      LOCUST_CHECK_ARG(!q.truth_at(0),
                       "search: the expression " + q.expr + " is true of a line that holds none of "
                       "its words (as NOT a, or a OR NOT b, is): the index cannot list such lines; "
                       "combine the NOT with a positive term (b AND NOT a)");
    }
    LOCUST_CHECK_ARG(!q.terms.empty() && q.terms.size() <= (size_t)kSearchMaxTerms,
                     "search: query " + std::to_string(i) + " has " +
                         std::to_string(q.terms.size()) + " terms; a query takes 1 to " +
                         std::to_string(kSearchMaxTerms) +
                         (q.excluded ? ", positive and exclusion terms together" : ""));
    LOCUST_CHECK_ARG((size_t)q.excluded < q.terms.size(),
                     "search: query " + std::to_string(i) + " has no positive term (" +
                         std::to_string(q.excluded) + " exclusion terms of " +
                         std::to_string(q.terms.size()) + "); exclusion terms take lines away "
                         "from what at least one positive term answers");
    for (size_t f = 1; f < q.files.size(); ++f)
      LOCUST_CHECK_ARG(q.files[f - 1] < q.files[f],
                       "search: the file set of query " + std::to_string(i) + " is not strictly "
                       "ascending (" + std::to_string(q.files[f - 1]) + " stands before " +
                       std::to_string(q.files[f]) + "): give distinct file ids in order");
    LOCUST_CHECK_ARG(q.prefix.empty() || q.prefix.size() == q.terms.size(),
                     "search: query " + std::to_string(i) + " has " +
                         std::to_string(q.prefix.size()) + " prefix flags for " +
                         std::to_string(q.terms.size()) + " terms; give none or one per term");
    if (q.mode == SearchMode::kNear)
      LOCUST_CHECK_ARG(q.within >= 1 && q.within <= kSearchMaxWithin,
                       "search: query " + std::to_string(i) + " is a near query: it takes a "
                       "window 1 <= W < 2^32 (within), not " + std::to_string(q.within));
    else
      LOCUST_CHECK_ARG(q.within == 0,
                       "search: query " + std::to_string(i) + " has a window (within " +
                           std::to_string(q.within) + ") but is no near query");
    LOCUST_CHECK_ARG(q.pattern.empty() || q.pattern.size() == q.terms.size(),
                     "search: query " + std::to_string(i) + " has " +
                         std::to_string(q.pattern.size()) + " pattern flags for " +
                         std::to_string(q.terms.size()) + " terms; give none or one per term");
    LOCUST_CHECK_ARG(q.fuzzy.empty() || q.fuzzy.size() == q.terms.size(),
                     "search: query " + std::to_string(i) + " has " +
                         std::to_string(q.fuzzy.size()) + " fuzzy budgets for " +
                         std::to_string(q.terms.size()) + " terms; give none or one per term");
    LOCUST_CHECK_ARG(q.regex.empty() || q.regex.size() == q.terms.size(),
                     "search: query " + std::to_string(i) + " has " +
                         std::to_string(q.regex.size()) + " regex flags for " +
                         std::to_string(q.terms.size()) + " terms; give none or one per term");
    for (size_t ti = 0; ti < q.terms.size(); ++ti) {
      const std::string& t = q.terms[ti];
      LOCUST_CHECK_ARG(!t.empty(), "search: query " + std::to_string(i) + " has an empty term");
      const bool pat = q.is_pattern(ti);
      if (q.is_regex(ti)) {
        LOCUST_CHECK_ARG(!q.is_prefix(ti) && !pat && !q.fuzzy_budget(ti),
                         "search: term " + std::to_string(ti) + " of query " + std::to_string(i) +
                             " is flagged as a regex term and as a prefix, pattern or fuzzy term; "
                             "it is one or the other");
        (void)compile_regex(t, false);  // (throws with the cause; a delimiter in it is legal)
        continue;
      }
      if (const u32 d = q.fuzzy_budget(ti)) {
        LOCUST_CHECK_ARG(!q.is_prefix(ti) && !pat,
                         "search: term " + std::to_string(ti) + " of query " + std::to_string(i) +
                             " is flagged as a fuzzy term and as a prefix or pattern term; it is "
                             "one or the other");
        LOCUST_CHECK_ARG(d <= kFuzzyMaxBudget,
                         "search: the fuzzy term " + t + " of query " + std::to_string(i) +
                             " has a budget of " + std::to_string(d) +
                             " edits; a budget is 1 or 2");
        LOCUST_CHECK_ARG(t.size() > (size_t)d,
                         "search: the fuzzy term " + t + "~" + std::to_string(d) + " of query " +
                             std::to_string(i) + " has a word of " + std::to_string(t.size()) +
                             " bytes; a fuzzy term's word is longer than its budget");
        LOCUST_CHECK_ARG(t.size() <= (size_t)cfg.max_key_len,
                         "search: the fuzzy term " + t + "~" + std::to_string(d) + " of query " +
                             std::to_string(i) + " has a word of " + std::to_string(t.size()) +
                             " bytes; a fuzzy term's word is never cut and takes at most "
                             "max_key_len = " + std::to_string(cfg.max_key_len));
      }
      if (pat) {
        LOCUST_CHECK_ARG(!q.is_prefix(ti), "search: term " + std::to_string(ti) + " of query " +
                                               std::to_string(i) +
                                               " is flagged as a prefix term and as a pattern "
                                               "term; it is one or the other");
        LOCUST_CHECK_ARG(t.size() <= (size_t)cfg.max_key_len,
                         "search: the pattern " + t + " of query " + std::to_string(i) + " has " +
                             std::to_string(t.size()) + " bytes; a pattern is never cut and "
                             "takes at most max_key_len = " + std::to_string(cfg.max_key_len));
        LOCUST_CHECK_ARG(t.find_first_not_of('*') != std::string::npos,
                         "search: a pattern of stars alone (query " + std::to_string(i) +
                             ") is no term: give at least one other byte (ham*, *ing, h?mlet)");
      }
      for (const char ch : t) {
        if (pat && (ch == '*' || ch == '?')) continue;  // a metacharacter, not a word's byte
        const unsigned char c = (unsigned char)ch;
        LOCUST_CHECK_ARG(c != 0 && c != '\n' && cfg.delimiters.find(ch) == std::string::npos,
                         "search: a term of query " + std::to_string(i) + " holds byte " +
                             std::to_string((unsigned)c) +
                             " (a NUL, a newline or a delimiter), which no word can hold");
      }
    }
  }
}

void check_search_merge(u64 queries, u64 elements) {
  if (elements >= (1ull << 32))
    throw Error("search: the prefix terms of the batch's " + std::to_string(queries) +
                " queries merge " + std::to_string(elements) +
                " list elements, which does not fit the 32-bit sort counter (2^32): split "
                "the batch");
}

bool search_term_pattern(const SearchQuery& q, size_t t, const JobConfig& cfg, bool ignore_case,
                         SearchPattern* out) {
  const bool pat = q.is_pattern(t);
  const u32 budget = q.fuzzy_budget(t);
  if (!pat && !budget && !ignore_case && !q.is_regex(t)) return false;
  if (!out) return true;
  const std::string& s = q.terms[t];
  out->rx.clear();
  out->src.clear();
  out->budget = 0;
  out->regex = false;
  if (q.is_regex(t)) {  // the program for the batch's fold; the source is the term's identity
    out->p = PackedKey{};
    out->meta = 0;
    out->regex = true;
    out->rx = compile_regex(s, ignore_case);
    out->src = s;
    return true;
  }
  char bytes[kKeyBytes];
  u32 meta = 0;
  int n = 0;
  if (budget) {  // the word as asked, every byte literal: never cut (check_search_queries)
    for (; n < (int)s.size() && n < kKeyBytes; ++n) bytes[n] = s[(size_t)n];
    if (ignore_case)
      for (int i = 0; i < n; ++i)
        if (bytes[i] >= 'A' && bytes[i] <= 'Z') bytes[i] = (char)(bytes[i] | 0x20);
    pack_key(bytes, n, out->p.w);
    out->meta = kFuzzyMeta | budget;  // (the device's meta word; the host reads `budget`)
    out->budget = budget;
    return true;
  }
  if (pat) {  // as asked: never cut (check_search_queries), star runs collapsed
    for (const char ch : s) {
      if (n == kKeyBytes) break;
      const bool m = ch == '*' || ch == '?';
      if (ch == '*' && n && bytes[n - 1] == '*' && ((meta >> (n - 1)) & 1u)) continue;
      if (m) meta |= 1u << n;
      bytes[n++] = ch;
    }
  } else {  // the cut term, every byte literal; a prefix term (after the cut) and its star
    const int len = (int)std::min<size_t>(s.size(), (size_t)cfg.max_key_len);
    for (; n < len && n < kKeyBytes; ++n) bytes[n] = s[(size_t)n];
    if (search_term_prefix(q, t, cfg) && n < kKeyBytes) {
      meta |= 1u << n;
      bytes[n++] = '*';
    }
  }
  if (ignore_case)
    for (int i = 0; i < n; ++i)
      if (!((meta >> i) & 1u) && bytes[i] >= 'A' && bytes[i] <= 'Z') bytes[i] = (char)(bytes[i] | 0x20);
  pack_key(bytes, n, out->p.w);
  out->meta = meta;
  return true;
}

bool search_has_patterns(const std::vector<SearchQuery>& queries, bool ignore_case) {
  if (ignore_case) return !queries.empty();
  for (const SearchQuery& q : queries)
    for (const u8 f : q.pattern)
      if (f) return true;
  return search_has_fuzzy(queries) || search_has_regex(queries);
}

bool search_has_regex(const std::vector<SearchQuery>& queries) {
  for (const SearchQuery& q : queries)
    for (const u8 f : q.regex)
      if (f) return true;
  return false;
}

bool search_has_fuzzy(const std::vector<SearchQuery>& queries) {
  for (const SearchQuery& q : queries)
    for (const u8 d : q.fuzzy)
      if (d) return true;
  return false;
}

void check_search_rank(u64 rank_k, const JobConfig& cfg, bool patterns) {
  if (rank_k == 0) return;
  LOCUST_CHECK_ARG(rank_k <= 0xffffffffull,
                   "search: rank takes 1 <= K < 2^32, not " + std::to_string(rank_k));
  LOCUST_CHECK_ARG(!patterns || (u64)cfg.emits_per_line <= kRankMaxEmits / kSearchMaxTerms,
                   "search: a ranked search with a pattern term (glob, fuzzy, ignore_case) takes "
                   "emits_per_line <= kRankMaxEmits / " + std::to_string(kSearchMaxTerms) + " = " +
                       std::to_string(kRankMaxEmits / kSearchMaxTerms) +
                       " (pattern terms' lists may overlap: a score reaches 32 * emits_per_line "
                       "* 8 and must fit 22 bits), not " + std::to_string(cfg.emits_per_line));
  LOCUST_CHECK_ARG((u64)cfg.emits_per_line <= kRankMaxEmits,
                   "search: a ranked search takes emits_per_line <= kRankMaxEmits = " +
                       std::to_string(kRankMaxEmits) + " (its scores fit 22 bits), not " +
                       std::to_string(cfg.emits_per_line));
}

void check_search_show(u64 show, u64 text_bytes) {
  if (show == 0) return;
  LOCUST_CHECK_ARG(show <= kShowMaxBytes,
                   "search: show takes 1 <= N <= " + std::to_string(kShowMaxBytes) +
                       " bytes per line, not " + std::to_string(show));
  LOCUST_CHECK_ARG(text_bytes < (1ull << 32),
                   "search: show takes a text window of less than 2^32 bytes (a span's start is "
                   "a u32), not " + std::to_string(text_bytes) + ": search a line window");
}

void check_search_by_file(u32 by_file, u64 rank_k, u64 show, u64 tally) {
  LOCUST_CHECK_ARG(by_file <= kByFileCount, "search: by_file takes kByFileNone, kByFile or "
                                            "kByFileCount, not " + std::to_string(by_file));
  LOCUST_CHECK_ARG(by_file != kByFileCount || (rank_k == 0 && show == 0 && tally == 0),
                   "search: count_only returns no line, so it goes with neither rank nor show nor "
                   "tally: ask for by_file to have the lines and the counts");
}

void check_search_tally(u64 tally) {
  if (tally == 0) return;
  LOCUST_CHECK_ARG(tally <= kTopKMax,
                   "search: tally takes 1 <= K <= kTopKMax = " + std::to_string(kTopKMax) +
                       " words per query, not " + std::to_string(tally) +
                       ": ask for fewer words (entries() of the index lists every word)");
}

TallyKeySplit tally_key_split(u64 n, u64 tokens) {
  const auto bit_length = [](u64 v) { return v ? 64u - (u32)__builtin_clzll(v) : 0u; };
  LOCUST_CHECK_ARG(tokens < (1ull << 32),
                   "search: the tally's returned lines hold " + std::to_string(tokens) +
                       " tokens, which does not fit the 32-bit pair counter (2^32): use --rank K "
                       "to return fewer lines, or fewer queries");
  TallyKeySplit ks;
  ks.r = bit_length(n ? n - 1 : 0);
  ks.c = bit_length(tokens);
  ks.cmask = ks.c ? (~0ull >> (64 - ks.c)) : 0ull;
  LOCUST_CHECK_ARG(ks.c + ks.r <= 54,
                   "search: the tally's rank key needs " + std::to_string(ks.c) +
                       " count bits (" + std::to_string(tokens) + " tokens) and " +
                       std::to_string(ks.r) + " rank bits (" + std::to_string(n) +
                       " index words), more than the 54 below the query: use --rank K to return "
                       "fewer lines, or fewer queries");
  return ks;
}

namespace {

// engine.hpp "tally": per query a bitmap of its returned lines, then one pass over the postings,
// word by word.  Needs no text.
void tally_lines(const IndexResult& x, u64 k, SearchResult* r) {
  const u64 t0 = now_ns();
  const size_t Q = r->queries.size();
  const size_t n = x.words.entries.size();
  const WordCountEntry* ent = x.words.entries.data();
  r->tally_k = k;
  r->tally_off.assign(1, 0);
  r->tally_words.assign(Q, 0);
  r->tally_tokens.assign(Q, 0);
  std::vector<u8> returned((size_t)r->num_lines, 0);
  std::vector<std::pair<u64, size_t>> counted;  // (count, word) of one query's words
  for (size_t q = 0; q < Q; ++q) {
    counted.clear();
    if (r->offsets[q + 1] > r->offsets[q]) {
      for (u64 e = r->offsets[q]; e < r->offsets[q + 1]; ++e)
        returned[(size_t)(r->lines[e] - r->first_line)] = 1;
      u64 at = 0;
      for (size_t w = 0; w < n; ++w) {
        u64 c = 0;
        for (const u64 end = at + ent[w].count; at < end; ++at)
          c += returned[(size_t)(x.postings[(size_t)at] - x.first_line)];
        if (c) counted.emplace_back(c, w);
        r->tally_tokens[q] += c;
      }
      for (u64 e = r->offsets[q]; e < r->offsets[q + 1]; ++e)
        returned[(size_t)(r->lines[e] - r->first_line)] = 0;
    }
    r->tally_words[q] = counted.size();
    // count descending, key ascending: the entries stand in key order, so a word's index decides
    const size_t take = (size_t)std::min<u64>(k, counted.size());
    std::partial_sort(counted.begin(), counted.begin() + (std::ptrdiff_t)take, counted.end(),
                      [](const auto& a, const auto& b) {
                        return a.first != b.first ? a.first > b.first : a.second < b.second;
                      });
    for (size_t i = 0; i < take; ++i) {
      r->tally_keys.push_back(ent[counted[i].second].key);
      r->tally_counts.push_back(counted[i].first);
    }
    r->tally_off.push_back(r->tally_keys.size());
  }
  r->tally_ms = (now_ns() - t0) * 1e-6;
  r->times.wall_ms += r->tally_ms;
}

// The positive terms a line's tokens are matched against.  masks: empty, or per key and word
// the bytes a token must share with it (a prefix term: key_word_mask of its words; a plain
// term: every byte).  pats: empty, or per key whether it is evaluated as a pattern term
// (is_pat) and then its pattern.
struct TokenTerms {
  std::vector<PackedKey> keys, masks;
  std::vector<SearchPattern> pats;
  std::vector<u8> is_pat;
  bool fold = false;
  size_t size() const { return keys.size(); }
};

// Does the token match term j?
bool token_matches(const PackedKey& tok, size_t j, const TokenTerms& tt) {
  if (!tt.pats.empty() && tt.is_pat[j])
    return tt.pats[j].matches(tok.w, tt.fold);
  if (tt.masks.empty()) return key_compare(tok.w, tt.keys[j].w) == 0;
  bool same = true;
  for (int i = 0; i < kKeyWords; ++i) same &= (tok.w[i] & tt.masks[j].w[i]) == tt.keys[j].w[i];
  return same;
}

// Do the first emits_per_line tokens of the line hold the keys as consecutive tokens?
bool line_has_phrase(const char* line, u64 len, const TokenTerms& keys, const JobConfig& cfg,
                     std::vector<PackedKey>* toks) {
  toks->clear();
  tokenize_line(line, len, cfg, toks, nullptr);
  const size_t m = keys.size();
  for (size_t o = 0; o + m <= toks->size(); ++o) {
    size_t j = 0;
    while (j < m && token_matches((*toks)[o + j], j, keys)) ++j;
    if (j == m) return true;
  }
  return false;
}

// Do `within` consecutive tokens among the first emits_per_line of the line match every key?
// Per key the position of its last matching token: the shortest window that ends at token o
// and covers every key starts at the smallest of them.
bool line_has_near(const char* line, u64 len, const TokenTerms& keys, u64 within,
                   const JobConfig& cfg, std::vector<PackedKey>* toks) {
  toks->clear();
  tokenize_line(line, len, cfg, toks, nullptr);
  const size_t m = keys.size();
  std::vector<size_t> last(m, (size_t)-1);
  for (size_t o = 0; o < toks->size(); ++o) {
    bool any = false;
    for (size_t j = 0; j < m; ++j)
      if (token_matches((*toks)[o], j, keys)) {
        last[j] = o;
        any = true;
      }
    if (!any) continue;
    size_t first = o;
    bool all = true;
    for (size_t j = 0; j < m && all; ++j) {
      all = last[j] != (size_t)-1;
      first = std::min(first, last[j]);
    }
    if (all && (u64)(o - first) < within) return true;
  }
  return false;
}

// The positive terms of q as a line's tokens are matched against them.
TokenTerms positive_terms(const SearchQuery& q, const JobConfig& cfg, bool patterns,
                          bool ignore_case) {
  TokenTerms keys;
  keys.fold = ignore_case;
  bool wild = false;
  const size_t npos = q.positives();
  for (size_t t = 0; t < npos; ++t) wild |= search_term_prefix(q, t, cfg);
  for (size_t t = 0; t < npos; ++t) {
    keys.keys.push_back(search_term_key(q.terms[t], cfg));
    if (patterns) {
      SearchPattern sp;
      keys.is_pat.push_back(search_term_pattern(q, t, cfg, ignore_case, &sp) ? 1 : 0);
      keys.pats.push_back(sp);
    }
    if (!wild) continue;
    PackedKey m;
    for (int j = 0; j < kKeyWords; ++j)
      m.w[j] = search_term_prefix(q, t, cfg) ? key_word_mask(keys.keys.back().w[j]) : ~0ull;
    keys.masks.push_back(m);
  }
  return keys;
}

// engine.hpp "show": the shown bytes and the spans of every entry of r, from the text.
void show_lines(const TextInput& text, const std::vector<u64>& line_at, const JobConfig& cfg,
                bool patterns, u32 show, SearchResult* r) {
  const u64 t0 = now_ns();
  r->show_bytes = show;
  r->text_off.assign(1, 0);
  r->span_off.assign(1, 0);
  std::vector<PackedKey> toks;
  std::vector<std::pair<u32, u32>> at;
  for (size_t qi = 0; qi < r->queries.size(); ++qi) {
    const TokenTerms keys = positive_terms(r->queries[qi], cfg, patterns, r->ignore_case);
    for (u64 e = r->offsets[qi]; e < r->offsets[qi + 1]; ++e) {
      const u64 l = r->lines[e] - r->first_line;
      LOCUST_CHECK_ARG(l + 1 < line_at.size(),
                       "search: the text has fewer lines than the index names");
      const char* p = text.data + line_at[l];
      u64 len = line_at[l + 1] - 1 - line_at[l];
      toks.clear();
      at.clear();
      tokenize_line(p, len, cfg, &toks, nullptr, &at);
      // (the text ends where the tokeniser stops: at a NUL, too)
      if (const void* nul = memchr(p, 0, (size_t)len))
        len = (u64)(static_cast<const char*>(nul) - p);
      r->cut_lines += len > show ? 1 : 0;
      r->text.append(p, (size_t)std::min<u64>(len, show));
      r->text_off.push_back(r->text.size());
      for (size_t o = 0; o < toks.size(); ++o) {
        u32 mask = 0;
        for (size_t j = 0; j < keys.size(); ++j) mask |= (u32)token_matches(toks[o], j, keys) << j;
        if (!mask) continue;
        r->spans.push_back(at[o].first);
        r->spans.push_back(at[o].second);
        r->spans.push_back(mask);
      }
      r->span_off.push_back(r->spans.size() / 3);
    }
  }
  r->show_ms = (now_ns() - t0) * 1e-6;
  r->times.wall_ms += r->show_ms;
}

SearchResult search_index_impl(const IndexResult& x, const TextInput* text,
                               const std::vector<SearchQuery>& queries, const JobConfig& cfg,
                               u64 rank_k, bool ignore_case, u64 show, u64 tally, u32 by_file) {
  check_search_queries(queries, cfg);
  check_search_by_file(by_file, rank_k, show, tally);
  const bool patterns = search_has_patterns(queries, ignore_case);
  check_search_rank(rank_k, cfg, patterns);
  LOCUST_CHECK_ARG(show == 0 || text,
                   "search: show needs the text (the index holds no bytes): use "
                   "search_index(index, text, queries, cfg, ...), the four-argument overload, or "
                   "run_search on an engine");
  check_search_show(show, text ? text->bytes : 0);
  check_search_tally(tally);
  bool verify = false;  // a phrase, or a near query, of two or more positive terms
  for (const SearchQuery& q : queries)
    verify |= (q.mode == SearchMode::kPhrase || q.mode == SearchMode::kNear) &&
              q.positives() >= 2;
  if (!text)
    for (const SearchQuery& q : queries) {
      LOCUST_CHECK_ARG(q.mode != SearchMode::kPhrase,
                       "search: a phrase query needs the text (the index holds no positions): "
                       "use search_index(index, text, queries, cfg), or run_search on an engine");
      LOCUST_CHECK_ARG(q.mode != SearchMode::kNear || q.positives() < 2,
                       "search: a near query of two or more terms needs the text (the index "
                       "holds no positions): use search_index(index, text, queries, cfg), or "
                       "run_search on an engine");
    }
  std::vector<u64> line_at;  // the text's line starts, and its size behind them
  if (verify || show) {
    LOCUST_CHECK_ARG(cfg.ngram == 1,
                     "search: a phrase or near query is verified, and a line shown, with word "
                     "keys (ngram 1)");
    LOCUST_CHECK_ARG(text->first_line == x.first_line && !text->source,
                     "search: the text is not the window the index was built from");
    for (u64 p = 0; p < text->bytes;) {
      line_at.push_back(p);
      const void* nl = memchr(text->data + p, '\n', (size_t)(text->bytes - p));
      p = nl ? (u64)(static_cast<const char*>(nl) - text->data) + 1 : text->bytes;
    }
    // (an end without a newline: the last line ends at bytes, not one before it)
    line_at.push_back(text->bytes && text->data[text->bytes - 1] != '\n' ? text->bytes + 1
                                                                         : text->bytes);
  }
  const u64 t0 = now_ns();
  SearchResult r;
  r.queries = queries;
  r.first_line = x.first_line;
  r.num_lines = x.words.num_lines;
  r.num_tokens = x.words.num_tokens;
  r.num_unique = x.words.num_unique;
  r.overflow_lines = x.words.overflow_lines;
  r.truncated = x.words.truncated;
  r.max_key_len = x.words.max_key_len;
  r.times = x.words.times;
  r.index_ms = x.index_ms;
  r.wire_bytes = x.wire_bytes;
  r.rank_k = rank_k;
  r.ignore_case = ignore_case;
  r.emits_per_line = (u64)cfg.emits_per_line;
  const IndexSegments table = x.segment_table();
  r.segments = table.segs;
  const size_t n = x.words.entries.size();
  const WordCountEntry* ent = x.words.entries.data();
  std::vector<u64> val(n + 1, 0);
  for (size_t i = 0; i < n; ++i) val[i + 1] = val[i] + ent[i].count;
  LOCUST_CHECK_ARG(val[n] == x.postings.size(), "search: the index's counts and postings disagree");
  r.offsets.assign(1, 0);
  r.term_counts.assign(queries.size() * kSearchMaxTerms, 0);
  struct List {
    const u32* p;
    u64 len;
    size_t lo, hi;  // the key range [lo, hi) of its words (a pattern term: lo == hi)
    bool is_pat;        // a pattern term, and its pattern
    SearchPattern pat;
  };
  std::vector<std::pair<u32, u32>> ranked;  // (score, line) of one query's matching lines
  for (size_t qi = 0; qi < queries.size(); ++qi) {
    const SearchQuery& q = queries[qi];
    const size_t from = r.lines.size();
    std::vector<List> lists;  // the present positive terms of distinct key ranges
    std::vector<List> not_lists;  // the present exclusion terms of distinct key ranges
    std::vector<std::vector<u32>> own;  // the merged lists of this query's prefix terms
    const size_t npos = q.positives();
    bool absent = false;
    std::vector<int> list_of(q.terms.size(), -1);  // kExpr: term t's list in `lists` (-1: absent)
    for (size_t t = 0; t < q.terms.size(); ++t) {
      const bool pos = t < npos;
      SearchPattern sp;
      if (search_term_pattern(q, t, cfg, ignore_case, &sp)) {
        // a pattern term: its words are scattered ranks, found by a scan with the matcher
        std::vector<List>& into = pos ? lists : not_lists;
        const List* same = nullptr;
        for (const List& o : into)
          if (o.is_pat && o.pat.same(sp)) same = &o;
        if (same) {  // repeats an earlier term: the same count, no second list
          r.term_counts[qi * kSearchMaxTerms + t] = same->len;
          if (pos) list_of[t] = (int)(same - lists.data());
          continue;
        }
        std::vector<size_t> words;
        u64 len = 0;
        for (size_t i = 0; i < n; ++i)
          if (sp.matches(ent[i].key.w, ignore_case)) {
            words.push_back(i);
            len += ent[i].count;
          }
        if (words.empty()) {
          // (an absent term is no list, so a later repetition scans again: absent again)
          absent |= pos;
          continue;
        }
        r.term_counts[qi * kSearchMaxTerms + t] = len;
        List l{x.postings.data() + val[words[0]], len, 0, 0, true, sp};
        if (words.size() >= 2) {
          own.emplace_back();
          own.back().reserve((size_t)len);
          for (const size_t w : words)
            own.back().insert(own.back().end(), x.postings.data() + val[w],
                              x.postings.data() + val[w + 1]);
          std::sort(own.back().begin(), own.back().end());
          l.p = own.back().data();
        }
        if (pos) list_of[t] = (int)lists.size();
        into.push_back(l);
        continue;
      }
      const PackedKey k = search_term_key(q.terms[t], cfg);
      const auto less = [](const WordCountEntry& a, const PackedKey& b) {
        return key_compare(a.key.w, b.w) < 0;
      };
      const size_t lo = (size_t)(std::lower_bound(ent, ent + n, k, less) - ent);
      size_t hi = lo;
      if (search_term_prefix(q, t, cfg)) {  // the keys from p padded with 0x00 to p with 0xff
        PackedKey top;
        for (int j = 0; j < kKeyWords; ++j) top.w[j] = k.w[j] | ~key_word_mask(k.w[j]);
        hi = (size_t)(std::upper_bound(ent, ent + n, top,
                                       [](const PackedKey& b, const WordCountEntry& a) {
                                         return key_compare(b.w, a.key.w) < 0;
                                       }) -
                      ent);
      } else if (lo < n && key_compare(ent[lo].key.w, k.w) == 0) {
        hi = lo + 1;
      }
      if (hi <= lo) {
        absent |= pos;  // (an absent exclusion term excludes nothing)
        continue;
      }
      r.term_counts[qi * kSearchMaxTerms + t] = val[hi] - val[lo];
      std::vector<List>& into = pos ? lists : not_lists;
      bool dup = false;
      for (const List& o : into) {
        if (o.is_pat || o.lo != lo || o.hi != hi) continue;
        dup = true;
        if (pos) list_of[t] = (int)(&o - lists.data());
      }
      if (dup) continue;
      List l{x.postings.data() + val[lo], val[hi] - val[lo], lo, hi, false, SearchPattern{}};
      if (hi - lo >= 2) {  // a concatenation of sorted lists: merge
        own.emplace_back(l.p, l.p + l.len);
        std::sort(own.back().begin(), own.back().end());
        l.p = own.back().data();
      }
      if (pos) list_of[t] = (int)lists.size();
      into.push_back(l);
    }
    // is the line one of the query's excluded lines?
    const auto excluded = [&](u32 line) {
      for (const List& l : not_lists)
        if (std::binary_search(l.p, l.p + l.len, line)) return true;
      return false;
    };
    // the score's terms: none whose key range lies inside another's (equal ranges are one
    // list here already)
    std::vector<List> scored;
    for (const List& l : lists) {
      bool inside = false;
      for (const List& o : lists)  // (pattern terms: inside nothing, and nothing inside them)
        inside |= &o != &l && !o.is_pat && !l.is_pat && o.lo <= l.lo && l.hi <= o.hi;
      if (!inside) scored.push_back(l);
    }
    if (q.mode == SearchMode::kExpr) {
      // "boolean expressions": every line of a present term's list, each once; its mask from
      // the terms' lists, the truth table decides (truth[0] is clear: no other line matches)
      for (const List& l : lists) r.lines.insert(r.lines.end(), l.p, l.p + l.len);
      std::sort(r.lines.begin() + (std::ptrdiff_t)from, r.lines.end());
      r.lines.erase(std::unique(r.lines.begin() + (std::ptrdiff_t)from, r.lines.end()),
                    r.lines.end());
      const auto no_match = [&](u32 line) {
        u32 in_list = 0, mask = 0;  // bit i: the line is in lists[i]; bit t: in term t's list
        for (size_t i = 0; i < lists.size(); ++i)
          in_list |= (u32)std::binary_search(lists[i].p, lists[i].p + lists[i].len, line) << i;
        for (size_t t = 0; t < q.terms.size(); ++t)
          if (list_of[t] >= 0) mask |= ((in_list >> list_of[t]) & 1u) << t;
        return !q.truth_at(mask);
      };
      r.lines.erase(std::remove_if(r.lines.begin() + (std::ptrdiff_t)from, r.lines.end(), no_match),
                    r.lines.end());
    } else if (q.mode != SearchMode::kAny) {
      const bool phrase = q.mode == SearchMode::kPhrase && npos >= 2;
      // (W >= emits_per_line: no line has more tokens, the `all` answer stands)
      const bool near = q.mode == SearchMode::kNear && npos >= 2 &&
                        q.within < (u64)cfg.emits_per_line;
      TokenTerms keys;
      std::vector<PackedKey> toks;
      if (phrase || near)  // the positive terms only
        keys = positive_terms(q, cfg, patterns, ignore_case);
      if (!absent && !lists.empty()) {
        size_t d = 0;
        for (size_t i = 1; i < lists.size(); ++i)
          if (lists[i].len < lists[d].len) d = i;
        for (u64 j = 0; j < lists[d].len; ++j) {
          const u32 line = lists[d].p[j];
          if (j && lists[d].p[j - 1] == line) continue;
          bool hit = true;
          for (size_t i = 0; i < lists.size() && hit; ++i)
            if (i != d) hit = std::binary_search(lists[i].p, lists[i].p + lists[i].len, line);
          hit = hit && !excluded(line);  // (before the line is read: the index decides)
          if (hit && (phrase || near)) {  // a candidate: the line itself decides
            const u64 l = line - x.first_line;
            LOCUST_CHECK_ARG(l + 1 < line_at.size(),
                             "search: the text has fewer lines than the index names");
            const char* at = text->data + line_at[l];
            const u64 len = line_at[l + 1] - 1 - line_at[l];
            hit = phrase ? line_has_phrase(at, len, keys, cfg, &toks)
                         : line_has_near(at, len, keys, q.within, cfg, &toks);
          }
          if (hit) r.lines.push_back(line);
        }
      }
    } else {
      for (const List& l : lists) r.lines.insert(r.lines.end(), l.p, l.p + l.len);
      std::sort(r.lines.begin() + (std::ptrdiff_t)from, r.lines.end());
      r.lines.erase(std::unique(r.lines.begin() + (std::ptrdiff_t)from, r.lines.end()),
                    r.lines.end());
      if (!not_lists.empty())
        r.lines.erase(std::remove_if(r.lines.begin() + (std::ptrdiff_t)from, r.lines.end(), excluded),
                      r.lines.end());
    }
    if (!q.files.empty()) {  // "file sets": the lines whose segment's id is in the set
      const auto outside = [&](u32 line) {
        return !std::binary_search(q.files.begin(), q.files.end(), table.segs[table.locate(line)].id);
      };
      r.lines.erase(std::remove_if(r.lines.begin() + (std::ptrdiff_t)from, r.lines.end(), outside),
                    r.lines.end());
    }
    r.matches.push_back(r.lines.size() - from);
    if (rank_k) {  // the matching lines' scores, the order and the cut
      const u64 N = x.postings.size();
      ranked.clear();
      for (size_t j = from; j < r.lines.size(); ++j) {
        const u32 line = r.lines[j];
        u64 score = 0;
        for (const List& l : scored) {
          const auto eq = std::equal_range(l.p, l.p + l.len, line);
          const u64 w = N / l.len;  // (>= 1: a list is part of the postings)
          score += (u64)(64 - __builtin_clzll(w)) * (u64)(eq.second - eq.first);
        }
        if (score == 0 || score > 32 * (u64)cfg.emits_per_line * (patterns ? kSearchMaxTerms : 1))
          throw Error("search: line " + std::to_string(line) + " of query " + std::to_string(qi) +
                      " scores " + std::to_string(score) + ", outside [1, 32 * emits_per_line" +
                      (patterns ? " * 8]" : "]"));
        ranked.emplace_back((u32)score, line);
      }
      std::sort(ranked.begin(), ranked.end(), [](const auto& a, const auto& b) {
        return a.first != b.first ? a.first > b.first : a.second < b.second;
      });
      if (ranked.size() > rank_k) ranked.resize((size_t)rank_k);
      r.lines.resize(from);
      for (const auto& sl : ranked) {
        r.lines.push_back(sl.second);
        r.scores.push_back(sl.first);
      }
    }
    r.offsets.push_back(r.lines.size());
  }
  r.search_ms = (now_ns() - t0) * 1e-6;
  r.times.wall_ms += r.search_ms;
  if (show) show_lines(*text, line_at, cfg, patterns, (u32)show, &r);
  if (tally) tally_lines(x, tally, &r);
  if (by_file) {  // "answers by file": every returned line's file, and the counts per query
    r.by_file = by_file;
    r.file_off.assign(1, 0);
    for (size_t qi = 0; qi < queries.size(); ++qi) {
      std::map<u32, u32> per;  // (ids ascend with the ordinals)
      for (u64 j = r.offsets[qi]; j < r.offsets[qi + 1]; ++j) {
        const IndexSegment& sg = table.segs[table.locate(r.lines[j])];
        r.line_file.push_back(sg.id);
        r.line_local.push_back((u32)(r.lines[j] - sg.first_line + sg.base));
        ++per[sg.id];
      }
      for (const auto& kv : per) {
        r.file_ids.push_back(kv.first);
        r.file_counts.push_back(kv.second);
      }
      r.file_off.push_back(r.file_ids.size());
    }
    if (by_file == kByFileCount) {  // the lines stay where they are: only the counts are answered
      r.lines.clear();
      r.line_file.clear();
      r.line_local.clear();
      r.offsets.assign(queries.size() + 1, 0);
    }
  }
  if (cfg.check) validate_search(r);
  return r;
}

}  // namespace

SearchResult search_index(const IndexResult& x, const std::vector<SearchQuery>& queries,
                          const JobConfig& cfg, u64 rank_k, bool ignore_case, u64 show,
                          u64 tally, u32 by_file) {
  return search_index_impl(x, nullptr, queries, cfg, rank_k, ignore_case, show, tally, by_file);
}

SearchResult search_index(const IndexResult& x, const TextInput& text,
                          const std::vector<SearchQuery>& queries, const JobConfig& cfg,
                          u64 rank_k, bool ignore_case, u64 show, u64 tally, u32 by_file) {
  return search_index_impl(x, &text, queries, cfg, rank_k, ignore_case, show, tally, by_file);
}

namespace {

// validate_search's part for engine.hpp "tally".
void validate_tally(const SearchResult& r) {
  if (r.tally_k == 0) {
    if (!r.tally_off.empty() || !r.tally_keys.empty() || !r.tally_counts.empty() ||
        !r.tally_words.empty() || !r.tally_tokens.empty() || r.tallied)
      throw Error("LOCUST_CHECK: search result without tally holds tallied words");
    return;
  }
  const size_t Q = r.queries.size();
  if (r.tally_k > kTopKMax)
    throw Error("LOCUST_CHECK: tally K = " + std::to_string(r.tally_k) + " above kTopKMax");
  if (r.tally_off.size() != Q + 1 || r.tally_off.front() != 0 ||
      r.tally_off.back() != r.tally_keys.size() || r.tally_counts.size() != r.tally_keys.size() ||
      r.tally_words.size() != Q || r.tally_tokens.size() != Q)
    throw Error("LOCUST_CHECK: tally offsets do not span the " +
                std::to_string(r.tally_keys.size()) + " words of " + std::to_string(Q) +
                " queries");
  for (size_t q = 0; q < Q; ++q) {
    if (r.tally_off[q + 1] < r.tally_off[q] || r.tally_off[q + 1] > r.tally_keys.size())
      throw Error("LOCUST_CHECK: tally offsets decrease at query " + std::to_string(q));
    const u64 got = r.tally_off[q + 1] - r.tally_off[q];
    if (got > std::min<u64>(r.tally_k, r.tally_words[q]))
      throw Error("LOCUST_CHECK: query " + std::to_string(q) + " tallies " + std::to_string(got) +
                  " words, more than min(K = " + std::to_string(r.tally_k) + ", " +
                  std::to_string(r.tally_words[q]) + " words)");
    if (r.tally_words[q] > r.tally_tokens[q] ||
        (r.tally_words[q] == 0) != (r.tally_tokens[q] == 0))
      throw Error("LOCUST_CHECK: query " + std::to_string(q) + " tallies " +
                  std::to_string(r.tally_words[q]) + " words over " +
                  std::to_string(r.tally_tokens[q]) + " tokens");
    u64 sum = 0;
    for (u64 j = r.tally_off[q]; j < r.tally_off[q + 1]; ++j) {
      const u64 c = r.tally_counts[j];
      if (c < 1)
        throw Error("LOCUST_CHECK: tallied word " + std::to_string(j - r.tally_off[q]) +
                    " of query " + std::to_string(q) + " has count 0");
      if (j > r.tally_off[q] &&
          (c > r.tally_counts[j - 1] ||
           (c == r.tally_counts[j - 1] &&
            key_compare(r.tally_keys[j - 1].w, r.tally_keys[j].w) >= 0)))
        throw Error("LOCUST_CHECK: tallied words of query " + std::to_string(q) +
                    " not in (count descending, key ascending) order at position " +
                    std::to_string(j - r.tally_off[q]));
      sum += c;
    }
    if (sum > r.tally_tokens[q])
      throw Error("LOCUST_CHECK: the tallied counts of query " + std::to_string(q) +
                  " add up to " + std::to_string(sum) + ", more than its " +
                  std::to_string(r.tally_tokens[q]) + " tokens");
  }
}

// validate_search's part for engine.hpp "answers by file".
void validate_by_file(const SearchResult& r, const IndexSegments& table) {
  if (r.by_file == kByFileNone) {
    if (!r.line_file.empty() || !r.line_local.empty() || !r.file_off.empty() ||
        !r.file_ids.empty() || !r.file_counts.empty())
      throw Error("LOCUST_CHECK: search result without by_file holds answers by file");
    return;
  }
  const size_t Q = r.queries.size();
  const bool count_only = r.by_file == kByFileCount;
  if (r.file_off.size() != Q + 1 || r.file_off.front() != 0 ||
      r.file_off.back() != r.file_ids.size() || r.file_counts.size() != r.file_ids.size() ||
      r.line_file.size() != r.lines.size() || r.line_local.size() != r.lines.size() ||
      (count_only && (!r.lines.empty() || r.rank_k || r.show_bytes || r.tally_k)))
    throw Error("LOCUST_CHECK: by-file offsets do not span the " +
                std::to_string(r.file_ids.size()) + " files of " + std::to_string(Q) +
                " queries, or its per-line arrays the " + std::to_string(r.lines.size()) +
                " lines");
  for (size_t j = 0; j < r.lines.size(); ++j) {  // ids and local numbers agree with the table
    const u64 l = r.lines[j];
    if (l < table.first_line || l >= table.first_line + table.num_lines) continue;  // (reported)
    const IndexSegment& sg = table.segs[table.locate(l)];
    if (r.line_file[j] != sg.id || r.line_local[j] != l - sg.first_line + sg.base)
      throw Error("LOCUST_CHECK: line " + std::to_string(l) + " is reported as line " +
                  std::to_string(r.line_local[j]) + " of file " + std::to_string(r.line_file[j]) +
                  ", the table says line " + std::to_string(l - sg.first_line + sg.base) +
                  " of file " + std::to_string(sg.id));
  }
  for (size_t q = 0; q < Q; ++q) {
    if (r.file_off[q + 1] < r.file_off[q] || r.file_off[q + 1] > r.file_ids.size())
      throw Error("LOCUST_CHECK: by-file offsets decrease at query " + std::to_string(q));
    u64 sum = 0;
    for (u64 f = r.file_off[q]; f < r.file_off[q + 1]; ++f) {
      if (r.file_counts[f] == 0 || (f > r.file_off[q] && r.file_ids[f] <= r.file_ids[f - 1]))
        throw Error("LOCUST_CHECK: files of query " + std::to_string(q) +
                    " not ascending, or one without a line, at position " +
                    std::to_string(f - r.file_off[q]));
      sum += r.file_counts[f];
    }
    const u64 returned = count_only ? r.matches[q] : r.offsets[q + 1] - r.offsets[q];
    if (sum != returned)
      throw Error("LOCUST_CHECK: the file counts of query " + std::to_string(q) + " add up to " +
                  std::to_string(sum) + ", it returns " + std::to_string(returned) + " lines");
    if (!count_only) {  // ... and they count the lines' own files
      std::map<u32, u64> per;
      for (u64 j = r.offsets[q]; j < r.offsets[q + 1]; ++j) ++per[r.line_file[j]];
      u64 f = r.file_off[q];
      for (const auto& kv : per) {
        if (f >= r.file_off[q + 1] || r.file_ids[f] != kv.first || r.file_counts[f] != kv.second)
          throw Error("LOCUST_CHECK: the file counts of query " + std::to_string(q) +
                      " disagree with its lines' files at file " + std::to_string(kv.first));
        ++f;
      }
    }
    // (under a file set every counted file is a selected one)
    const std::vector<u32>& fs = r.queries[q].files;
    for (u64 f = r.file_off[q]; !fs.empty() && f < r.file_off[q + 1]; ++f)
      if (!std::binary_search(fs.begin(), fs.end(), r.file_ids[f]))
        throw Error("LOCUST_CHECK: query " + std::to_string(q) + " counts file " +
                    std::to_string(r.file_ids[f]) + ", outside its file set");
  }
}

}  // namespace

void validate_search(const SearchResult& r) {
  if (r.offsets.size() != r.queries.size() + 1 || r.offsets.front() != 0 ||
      r.offsets.back() != r.lines.size())
    throw Error("LOCUST_CHECK: search offsets do not span the " + std::to_string(r.lines.size()) +
                " lines of " + std::to_string(r.queries.size()) + " queries");
  if (r.matches.size() != r.queries.size() ||
      r.scores.size() != (r.rank_k ? r.lines.size() : (size_t)0))
    throw Error("LOCUST_CHECK: search result with " + std::to_string(r.matches.size()) +
                " match counts and " + std::to_string(r.scores.size()) + " scores for " +
                std::to_string(r.queries.size()) + " queries and " +
                std::to_string(r.lines.size()) + " lines");
  const u64 lo = r.first_line, hi = r.first_line + r.num_lines;
  // (pattern terms' lists may overlap: one token may count for every term of a query)
  const u64 score_max = 32 * r.emits_per_line *
                        (search_has_patterns(r.queries, r.ignore_case) ? kSearchMaxTerms : 1);
  IndexSegments table;  // "file sets": under a set, every line lies in a selected file
  table.reset(r.first_line, r.num_lines);
  if (!r.segments.empty()) table.segs = r.segments;
  for (size_t q = 0; q + 1 < r.offsets.size(); ++q) {
    if (r.offsets[q + 1] < r.offsets[q] || r.offsets[q + 1] > r.lines.size())
      throw Error("LOCUST_CHECK: search offsets decrease at query " + std::to_string(q));
    const std::vector<u32>& fs = r.queries[q].files;
    for (u64 j = r.offsets[q]; !fs.empty() && j < r.offsets[q + 1]; ++j) {
      const u64 l = r.lines[j];
      if (l < lo || l >= hi) continue;  // (reported below)
      const u32 id = table.segs[table.locate(l)].id;
      if (!std::binary_search(fs.begin(), fs.end(), id))
        throw Error("LOCUST_CHECK: line " + std::to_string(l) + " of query " + std::to_string(q) +
                    " lies in file " + std::to_string(id) + ", outside the query's file set");
    }
    const u64 returned = r.offsets[q + 1] - r.offsets[q];
    if (r.by_file == kByFileCount ? returned != 0 : r.rank_k ? returned > std::min<u64>(r.rank_k, r.matches[q]) : returned != r.matches[q])
      throw Error("LOCUST_CHECK: query " + std::to_string(q) + " returns " +
                  std::to_string(returned) + " lines of " + std::to_string(r.matches[q]) +
                  " matches");
    for (u64 j = r.offsets[q]; j < r.offsets[q + 1]; ++j) {
      const u64 l = r.lines[j];
      if (l < lo || l >= hi)
        throw Error("LOCUST_CHECK: line " + std::to_string(l) + " of query " + std::to_string(q) +
                    " outside the lines [" + std::to_string(lo) + ", " + std::to_string(hi) + ")");
      if (r.rank_k) {
        const u64 sc = r.scores[j];
        if (sc < 1 || sc > score_max)
          throw Error("LOCUST_CHECK: score " + std::to_string(sc) + " of query " +
                      std::to_string(q) + " outside [1, " + std::to_string(score_max) + "]");
        if (j > r.offsets[q] &&
            (sc > r.scores[j - 1] || (sc == r.scores[j - 1] && l <= r.lines[j - 1])))
          throw Error("LOCUST_CHECK: lines of query " + std::to_string(q) +
                      " not in rank order at position " + std::to_string(j - r.offsets[q]));
        continue;
      }
      if (j > r.offsets[q] && l <= r.lines[j - 1])
        throw Error("LOCUST_CHECK: lines of query " + std::to_string(q) +
                    " not strictly ascending at position " + std::to_string(j - r.offsets[q]));
    }
  }
  validate_tally(r);
  validate_by_file(r, table);
  if (r.show_bytes == 0) {
    if (!r.text.empty() || !r.text_off.empty() || !r.spans.empty() || !r.span_off.empty() ||
        r.cut_lines)
      throw Error("LOCUST_CHECK: search result without show holds shown lines");
    return;
  }
  const size_t E = r.lines.size();
  if (r.text_off.size() != E + 1 || r.text_off.front() != 0 || r.text_off.back() != r.text.size())
    throw Error("LOCUST_CHECK: show text offsets do not span the " + std::to_string(r.text.size()) +
                " bytes of " + std::to_string(E) + " entries");
  if (r.span_off.size() != E + 1 || r.span_off.front() != 0 || r.spans.size() % 3 != 0 ||
      r.span_off.back() != r.spans.size() / 3)
    throw Error("LOCUST_CHECK: show span offsets do not span the " +
                std::to_string(r.spans.size() / 3) + " spans of " + std::to_string(E) + " entries");
  if (r.cut_lines > E)
    throw Error("LOCUST_CHECK: " + std::to_string(r.cut_lines) + " cut lines of " +
                std::to_string(E) + " entries");
  for (size_t q = 0; q + 1 < r.offsets.size(); ++q) {
    const u32 npos = (u32)r.queries[q].positives();
    for (u64 e = r.offsets[q]; e < r.offsets[q + 1]; ++e) {
      if (r.text_off[e + 1] < r.text_off[e] || r.text_off[e + 1] - r.text_off[e] > r.show_bytes ||
          r.text_off[e + 1] > r.text.size())
        throw Error("LOCUST_CHECK: entry " + std::to_string(e) + " shows " +
                    std::to_string(r.text_off[e + 1] - r.text_off[e]) + " bytes, N = " +
                    std::to_string(r.show_bytes));
      if (r.span_off[e + 1] < r.span_off[e] || r.span_off[e + 1] > r.spans.size() / 3)
        throw Error("LOCUST_CHECK: show span offsets decrease at entry " + std::to_string(e));
      // a line shorter than N is shown whole: its spans lie inside the shown bytes
      const u64 tl = r.text_off[e + 1] - r.text_off[e];
      const u64 line_max = tl < r.show_bytes ? tl : (1ull << 32);
      u64 from = 0;  // the end of the span before
      for (u64 s = r.span_off[e]; s < r.span_off[e + 1]; ++s) {
        const u64 st = r.spans[3 * s], ln = r.spans[3 * s + 1];
        const u32 mask = r.spans[3 * s + 2];
        if (ln == 0 || st < from || (s > r.span_off[e] && st == from) || st + ln > line_max)
          throw Error("LOCUST_CHECK: span " + std::to_string(s - r.span_off[e]) + " of entry " +
                      std::to_string(e) + " (" + std::to_string(st) + ", " + std::to_string(ln) +
                      ") overlaps the span before it or leaves the line");
        if (mask == 0 || (npos < 32 && (mask >> npos) != 0))
          throw Error("LOCUST_CHECK: span " + std::to_string(s - r.span_off[e]) + " of entry " +
                      std::to_string(e) + " has mask " + std::to_string(mask) + " for " +
                      std::to_string(npos) + " positive terms");
        from = st + ln;
      }
    }
  }
}

void format_search_output(const SearchResult& r, std::string* out, bool mark) {
  out->reserve(out->size() + r.queries.size() * 48 + r.lines.size() * 6 + r.text.size() +
               r.lines.size() * 16);
  for (size_t q = 0; q < r.queries.size(); ++q) {
    out->append("print query:");
    const size_t npos = r.queries[q].positives();
    const bool expr = r.queries[q].mode == SearchMode::kExpr;
    if (expr) {  // the expression as asked, where the other modes print the joined terms
      out->push_back(' ');
      out->append(r.queries[q].expr);
    }
    for (size_t t = 0; !expr && t < r.queries[q].terms.size(); ++t) {
      if (t == npos) out->append(" \t not:");
      out->push_back(' ');
      if (r.queries[q].is_regex(t)) out->push_back('/');
      out->append(r.queries[q].terms[t]);
      if (r.queries[q].is_regex(t)) out->push_back('/');
      if (r.queries[q].is_prefix(t)) out->push_back('*');
      if (const u32 d = r.queries[q].fuzzy_budget(t)) {
        out->push_back('~');
        out->push_back((char)('0' + d));
      }
    }
    out->append(" \t hits: ");
    out->append(std::to_string(r.rank_k ? r.matches[q] : r.offsets[q + 1] - r.offsets[q]));
    out->append(r.rank_k ? " \t top:" : " \t lines:");
    for (u64 j = r.offsets[q]; j < r.offsets[q + 1]; ++j) {
      out->push_back(' ');
      out->append(std::to_string(r.lines[j]));
      if (r.rank_k) {
        out->push_back(':');
        out->append(std::to_string(r.scores[j]));
      }
    }
    out->push_back('\n');
    for (u64 e = r.offsets[q]; r.show_bytes && e < r.offsets[q + 1]; ++e) {
      out->append("  ");
      out->append(std::to_string(r.lines[e]));
      out->append(": ");
      const char* t = r.text.data() + r.text_off[e];
      const u64 tl = r.text_off[e + 1] - r.text_off[e];
      u64 done = 0;
      if (mark)
        for (u64 s = r.span_off[e]; s < r.span_off[e + 1]; ++s) {
          const u64 st = r.spans[3 * s], en = std::min<u64>(st + r.spans[3 * s + 1], tl);
          if (st >= tl) break;  // (ascending: the spans behind it lie outside the shown bytes too)
          out->append(t + done, (size_t)(st - done));
          out->append(">>");
          out->append(t + st, (size_t)(en - st));
          out->append("<<");
          done = en;
        }
      out->append(t + done, (size_t)(tl - done));
      out->push_back('\n');
    }
    if (!r.tally_k) continue;
    out->append("  words: ");
    out->append(std::to_string(r.tally_words[q]));
    out->append(" \t tokens: ");
    out->append(std::to_string(r.tally_tokens[q]));
    out->push_back('\n');
    char buf[kKeyBytes + 1];
    for (u64 j = r.tally_off[q]; j < r.tally_off[q + 1]; ++j) {
      const int kn = unpack_key(r.tally_keys[j].w, buf);
      out->append("  word: ");
      out->append(buf, (size_t)kn);
      out->append(" \t count: ");
      out->append(std::to_string(r.tally_counts[j]));
      out->push_back('\n');
    }
  }
}

}  // namespace locust
