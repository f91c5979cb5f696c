// WordCount engines: the single-GPU HIP pipeline and the CPU reference pipeline.
//
// GpuWordCount reproduces the reference's GPU path (/root/reference/
// MapReduce/src/main.cu:388-487) stage for stage -- Map (tokenize/emit), Process
// (stream compaction + key sort), Reduce (boundary mark + head compaction + adjacent
// difference) -- with every buffer preallocated at construction so a run performs no
// allocation and, apart from reading back result sizes, no host synchronisation.
// CpuWordCount is the golden oracle and the `--backend cpu` path (main.cu:489-527).
#pragma once

#include <array>
#include <cstddef>
#include <iterator>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "locust/common.hpp"
#include "locust/config.hpp"
#include "locust/kv.hpp"

namespace locust {

// A window of input lines: `bytes` bytes of text, lines separated by '\n' (the last line
// may lack one).  `first_line` is the global index of the first line (the reference's
// KeyValuePair.key, main.cu:58).
class TextSource;
struct TextInput {
  const char* data = nullptr;
  u64 bytes = 0;
  u64 num_lines = 0;
  u64 first_line = 0;
  // Distributed shards only: a shard larger than one device pass may be streamed from a
  // source (a rank's byte range of a file) instead of held in memory -- data is then null,
  // bytes the range's size, and num_lines unknown until the source is drained.
  TextSource* source = nullptr;
  u64 lines() const;  // num_lines, or the lines the source has handed out
};

struct StageTimes {
  // Honest device time from hipEvents on the compute stream (ms).
  double h2d_ms = 0, map_ms = 0, process_ms = 0, reduce_ms = 0, d2h_ms = 0;
  // Host wall clock of the whole run() call (ms).
  double wall_ms = 0;
  // Device time of the whole job (first to last enqueued operation, hipEvents).
  double gpu_ms = 0;
  // Host-side split of wall_ms (single-GPU runs): enqueue/launch, waiting for the device,
  // and copying the results out of the host-mapped output.
  double host_launch_ms = 0, host_wait_ms = 0, host_copy_ms = 0;
  bool graph = false;  // replayed as one hipGraph: the stage fields above are not split
  bool lean = false;   // direct launches, polled completion: no device stage timestamps
  // Host timers placed where the reference placed them (launch-only map etc., BASELINE.md
  // "How the reference measured these"), filled when JobConfig.ref_timers is set.
  double ref_map_ms = 0, ref_process_ms = 0, ref_reduce_ms = 0;
};

// One output entry: a unique key and the length of its run in the globally sorted token
// array (`count`); 40 B, the layout of KeyCount and of the device's output records.  The
// reference's `val` (start index of the run, KeyValue.h:13-18 / main.cu:181-206) is the
// exclusive prefix of the counts in key order: it is not stored per entry (it would be 8 B
// of every record crossing PCIe) but rebuilt on the host from WordCountResult::val_base --
// see EntryVals.
struct WordCountEntry {
  PackedKey key;
  u64 count;
};
static_assert(sizeof(WordCountEntry) == 40, "WordCountEntry 40 B");

// One segment of compact records (kv.hpp CompactRecord: a header word, then the key's
// non-zero words) holding `n` entries in key order.
struct EntrySegment {
  const u64* words = nullptr;
  u64 n = 0;
};

// The entries of a result: an owned vector, or -- zero-copy -- the engine's host-mapped
// output buffer itself, which the device wrote and which this list keeps alive (`owner`)
// until it is dropped; the engine then reuses the buffer for a later job.  The device may
// have written that buffer as 40-B records (adopt) or as compact records (adopt_compact:
// segments in key order, ~16-24 B per entry).  Iteration decodes
// compact records on the fly; data() / operator[] turn a compact list into an owned
// vector first (once).  Vector-like.
class EntryList {
 public:
  EntryList() = default;
  EntryList(std::vector<WordCountEntry>&& v) : vec_(std::move(v)) {}  // NOLINT: implicit
  EntryList& operator=(std::vector<WordCountEntry>&& v) {
    release();
    vec_ = std::move(v);
    return *this;
  }
  // Borrow n entries at p, kept valid by `owner`.
  void adopt(std::shared_ptr<void> owner, WordCountEntry* p, size_t n) {
    release();
    vec_.clear();
    vec_.shrink_to_fit();
    owner_ = std::move(owner);
    view_ = p;
    n_ = n;
  }
  // Borrow compact segments (n entries in all), kept valid by `owner`.
  void adopt_compact(std::shared_ptr<void> owner, std::vector<EntrySegment> segs, size_t n) {
    adopt(std::move(owner), nullptr, n);
    segs_ = std::move(segs);
    compact_ = true;
  }
  bool borrowed() const { return owner_ != nullptr; }
  bool compact() const { return compact_; }
  size_t size() const { return owner_ ? n_ : vec_.size(); }
  bool empty() const { return size() == 0; }
  // Bytes the device wrote for these entries (compact: the segments' words).
  u64 wire_bytes() const;
  WordCountEntry* data() {
    materialize();
    return owner_ ? view_ : vec_.data();
  }
  const WordCountEntry* data() const {
    materialize();
    return owner_ ? view_ : vec_.data();
  }
  WordCountEntry& operator[](size_t i) { return data()[i]; }
  const WordCountEntry& operator[](size_t i) const { return data()[i]; }
  WordCountEntry front() const { return *begin(); }

  // Forward iteration over either form; yields entries by value.
  class const_iterator {
   public:
    using iterator_category = std::forward_iterator_tag;
    using value_type = WordCountEntry;
    using difference_type = std::ptrdiff_t;
    using pointer = const WordCountEntry*;
    using reference = WordCountEntry;
    const_iterator() = default;
    WordCountEntry operator*() const {
      if (flat_) return *flat_;
      WordCountEntry e;
      decode_compact(w_, &e.key, &e.count);
      return e;
    }
    const_iterator& operator++() {
      if (flat_) {
        ++flat_;
        return *this;
      }
      w_ += compact_record_words(w_[0]);
      if (--left_ == 0) next_segment();
      return *this;
    }
    const_iterator operator++(int) {
      const_iterator t = *this;
      ++*this;
      return t;
    }
    bool operator==(const const_iterator& o) const { return flat_ == o.flat_ && w_ == o.w_; }
    bool operator!=(const const_iterator& o) const { return !(*this == o); }

   private:
    friend class EntryList;
    void next_segment() {
      w_ = nullptr;
      while (seg_ != seg_end_) {
        const EntrySegment& s = *seg_++;
        if (s.n) {
          w_ = s.words;
          left_ = s.n;
          return;
        }
      }
    }
    const WordCountEntry* flat_ = nullptr;
    const u64* w_ = nullptr;
    u64 left_ = 0;
    const EntrySegment* seg_ = nullptr;
    const EntrySegment* seg_end_ = nullptr;
  };
  const_iterator begin() const {
    const_iterator it;
    if (compact_) {
      it.seg_ = segs_.data();
      it.seg_end_ = segs_.data() + segs_.size();
      it.next_segment();
    } else if (size()) {
      it.flat_ = owner_ ? view_ : vec_.data();
    }
    return it;
  }
  const_iterator end() const {
    const_iterator it;
    if (!compact_ && size()) it.flat_ = (owner_ ? view_ : vec_.data()) + size();
    return it;
  }
  // Owned storage of n entries (a borrowed prefix is copied over).
  void resize(size_t n) {
    if (owner_) {
      std::vector<WordCountEntry> v;
      v.reserve(n);
      for (auto it = begin(); it != end() && v.size() < n; ++it) v.push_back(*it);
      release();
      vec_ = std::move(v);
    }
    vec_.resize(n);
  }
  void assign(const WordCountEntry* b, const WordCountEntry* e) {
    release();
    vec_.assign(b, e);
  }

 private:
  void release() const {
    owner_.reset();
    view_ = nullptr;
    n_ = 0;
    segs_.clear();
    compact_ = false;
  }
  // compact -> an owned vector (the buffer is released)
  void materialize() const {
    if (!compact_) return;
    std::vector<WordCountEntry> v;
    v.reserve(n_);
    for (auto it = begin(); it != end(); ++it) v.push_back(*it);
    release();
    vec_ = std::move(v);
  }
  mutable std::vector<WordCountEntry> vec_;
  mutable std::shared_ptr<void> owner_;
  mutable WordCountEntry* view_ = nullptr;
  mutable size_t n_ = 0;
  mutable std::vector<EntrySegment> segs_;
  mutable bool compact_ = false;
};

struct WordCountResult {
  EntryList entries;  // sorted by key
  // val of entries[0]: 0 for a whole result, the token total of the lower ranks' key
  // ranges for one rank's range of a distributed job.
  u64 val_base = 0;
  u64 num_lines = 0;
  u64 num_tokens = 0;       // kv_num_map
  u64 num_unique = 0;       // kv_num_reduce
  u64 overflow_lines = 0;   // lines that printed "WARN: Exceeded emit limit"
  u64 truncated = 0;        // tokens longer than max_key_len
  u64 max_key_len = 0;
  u64 chunks = 1;           // > 1: the input streamed through the engine in chunks
  StageTimes times;
};

// The reference's val of each entry in order: val(i) = val_base + sum of counts before i.
//   EntryVals v(res); for (auto& e : res.entries) { u64 val = v.next(e); ... }
class EntryVals {
 public:
  explicit EntryVals(const WordCountResult& r) : at_(r.val_base) {}
  explicit EntryVals(u64 base) : at_(base) {}
  u64 next(const WordCountEntry& e) {
    const u64 v = at_;
    at_ += e.count;
    return v;
  }

 private:
  u64 at_;
};

// ---- top-K words by count ----
// top(K) of a WordCount result: the min(K, num_unique) entries with the largest count, in
// rank order -- count descending, ties by key ascending (unsigned-byte order: the entry's
// index in the key-ordered output).  The order is total, so the answer is unique.  Every
// entry keeps the val it has in the full output (the exclusive prefix of the counts in key
// order): the top-K lines are a reordered subset of the full output's lines.
//
// The device selection (kernels/topk.hip; GpuWordCount::run_top) takes K <= kTopKMax: the
// final ordering of the winners is one workgroup's LDS sort.  The host selection
// (top_entries) takes any K.
constexpr u32 kTopKMax = 4096;
constexpr u32 kTopKTile = 2048;  // records per workgroup of the selection kernels

// ---- word n-grams (JobConfig::ngram) ----
// One record per n-gram of a line: N consecutive words joined by single 0x20 bytes.  N = 1
// is the word job.  Every engine refuses a value outside [1, kMaxNgram].
constexpr int kMaxNgram = 3;
// Throws unless cfg.ngram is in [1, kMaxNgram] (the engine constructors' check).
void check_ngram(const JobConfig& cfg);

struct TopEntry {
  PackedKey key;
  u64 count;
  u64 val;
};
static_assert(sizeof(TopEntry) == 48, "TopEntry 48 B (the device's TopRecord)");

struct TopResult {
  std::vector<TopEntry> entries;  // rank order
  u64 k = 0;                      // the K asked for
  // the whole job's statistics, as in WordCountResult
  u64 num_lines = 0;
  u64 num_tokens = 0;
  u64 num_unique = 0;
  u64 overflow_lines = 0;
  u64 truncated = 0;
  u64 max_key_len = 0;
  u64 chunks = 1;
  StageTimes times;
  double select_ms = 0;  // device time of the selection (0: selected on the host)
  u64 wire_bytes = 0;    // bytes the device wrote to host memory for the result
};

// Host selection, any k: partial sort over either entry form, val rebuilt with EntryVals.
std::vector<TopEntry> top_entries(const WordCountResult& r, u64 k);
// ... with the job's statistics carried over.
TopResult top_result(const WordCountResult& r, u64 k);
// LOCUST_CHECK invariants of a top result: min(k, num_unique) entries, counts
// non-increasing, ties key-ascending.
void validate_top(const TopResult& t);
// The result lines of a top result, in rank order: the GPU build's (with val) or the CPU
// build's (format_gpu_output / format_cpu_output, io.hpp).
void format_top_output(const TopResult& t, bool cpu_format, std::string* out);

// ---- corpus: several files in one index ----
// A resident index is cut into S >= 1 segments: consecutive, possibly empty, line ranges that
// cover [first_line, first_line + num_lines) in order -- the files of a corpus.  A segment has
// an id (a u32 that numbers the files in the order they were begun: run_index / run_search begin
// file 0, append_index(new_file) the next; a dropped file never frees its id), first_line (the
// global number of its first resident line) and base (the file-local number of that line: 0
// until a drop cuts into the file).  A global line l belongs to the LAST segment with
// first_line <= l, so an empty file between two others owns no line; its local number is
// l - first_line + base, 0-based like every line number here.
//  * append(lines, new_file): with new_file a segment with the next id begins at the block's
//    first line; without it the block extends the last segment.  More than kCorpusMaxFiles
//    resident segments are refused, the table unchanged.
//  * drop(d): segments that lie wholly inside the dropped lines leave the table (the non-empty
//    ones are counted and returned); the segment the cut falls into keeps its id, its first_line
//    becomes F + d and its base grows by the lines it lost; empty segments in front of the first
//    resident line go with the dropped ones.  d == N leaves the last segment, empty, so the
//    next block without new_file continues that file's numbering.  d == 0 changes nothing.
//  * locate(l): the ordinal of l's segment (l inside the resident lines).
// The table is host state of an engine; the host twins (merge_index, trim_index, search_index)
// carry it in IndexResult::segments, where an empty table stands for the single segment
// (0, first_line, 0).
constexpr u64 kCorpusMaxFiles = 65536;
struct IndexSegment {
  u32 id = 0;
  u64 first_line = 0;
  u64 base = 0;
  bool operator==(const IndexSegment& o) const {
    return id == o.id && first_line == o.first_line && base == o.base;
  }
};
struct IndexSegments {
  std::vector<IndexSegment> segs;  // never empty behind reset()
  u64 first_line = 0, num_lines = 0;
  u32 next_id = 0;
  void reset(u64 first, u64 lines);
  void append(u64 lines, bool new_file);
  u64 drop(u64 lines);
  size_t locate(u64 line) const;
  // the resident lines of segment i
  u64 lines_of(size_t i) const {
    return (i + 1 < segs.size() ? segs[i + 1].first_line : first_line + num_lines) -
           segs[i].first_line;
  }
  // the ordinal of the resident segment with this id, or segs.size()
  size_t find(u32 id) const;
};

// ---- inverted index: word -> the lines it occurs on ----
// Every token the word job emits (its tokeniser, emit cap and key truncation, unchanged)
// yields one pair (key, line); `line` is the global 0-based line number first_line + i.
// The pairs are sorted by (key in unsigned-byte order, line ascending).  The result is the
// word job's entries for the same input and configuration, and `postings`: one u32 line
// number per emitted token in sorted pair order -- entry i's list is
// postings[val_i .. val_i + count_i), non-decreasing, with val the reference's val (the
// exclusive prefix of the counts: EntryVals).  A word that occurs twice on a line has that
// line twice, so the list's length is the count and postings.size() == num_tokens.  Long
// tokens that merge under truncation merge their lists.  Word keys only (ngram == 1).
struct IndexResult {
  WordCountResult words;       // the word job: entries, statistics, stage times
  std::vector<u32> postings;   // line numbers, CSR-indexed by the entries' (val, count)
  u64 first_line = 0;          // the input window's first line (postings start there)
  double index_ms = 0;         // device time of the index stage (0: built on the host)
  u64 wire_bytes = 0;          // bytes the device wrote to host memory for the result
  std::vector<IndexSegment> segments;  // "corpus" above; empty: the one segment (0, first_line, 0)
  // the table as IndexSegments (an empty one made whole)
  IndexSegments segment_table() const;
};
// LOCUST_CHECK invariants of an index result: the entries' counts add up to
// postings.size() == num_tokens, every list is non-decreasing, every posting lies in
// [first_line, first_line + num_lines).
void validate_index(const IndexResult& r);
// The result lines of an index, in key order:
//   "print key: <key> \t count: <count> \t lines: <l0> <l1> ...\n"
void format_index_output(const IndexResult& r, std::string* out);

// ---- appending to the index ----
// An index may be built block by block.  After run_index(t0) (or run_search), then
// append_index(t1), ..., append_index(tk), the index in device memory is exactly the index of
// the text t0 + t1 + ... + tk with t0's first_line: the same records, postings, text and line
// starts a single pass over the concatenation would have left, so every search answers the
// same.  A block is whole lines numbered behind all resident lines, so for every word the
// merged postings list is the resident list followed by the block's: the block is indexed by
// the one-pass kernels, then merged with the resident index on the device (kernels/
// append.hip), a linear pass.  The text need not fit one pass any more, only device memory.
//  * Refused before anything is enqueued, the resident index intact and still searchable: no
//    resident index or a stale one; a block whose first_line is not the resident first_line +
//    lines; a block larger than the engine's pass; a resident text that is non-empty and does
//    not end in '\n' (the concatenation would join two lines); line numbers past 2^32.
//  * Any failure after the block's job has started leaves the index stale, merged totals of
//    2^32 tokens or words included.
//  * An empty block and an empty resident text are legal; the last block may lack its '\n'.
// Only counters cross PCIe.
struct IndexAppend {
  u64 block_lines = 0, block_tokens = 0, block_unique = 0;  // the block's own index
  u64 num_lines = 0, num_tokens = 0, num_unique = 0;        // the resident index after the merge
  u64 fresh_words = 0;    // words of the block the resident index did not hold
  double index_ms = 0;    // device time of the block's index stage
  double append_ms = 0;   // device time of the merge
  StageTimes times;       // the block's word job
  u64 store_bytes = 0;    // device bytes of the index store (both halves and the merge's scratch)
  u64 files = 0;          // resident segments afterwards ("corpus")
};
// The host twin of the device merge: the index of a's text followed by b's, from the two
// indexes alone, with the same checks (keys strictly ascending on either side, the counts
// adding up to the postings).  Throws unless b.first_line == a.first_line + a.words.num_lines.
// new_file: b begins a segment with a's next id ("corpus"); else it extends a's last segment.
// b's own table is not looked at: b is one block.
IndexResult merge_index(const IndexResult& a, const IndexResult& b, bool new_file = false);

// ---- dropping the oldest lines ----
// The mirror image of an append, for an index that follows a log or a feed and is searched
// over its most recent part.  The resident index holds the lines [F, F + N).  After
// drop_index(d) with 0 <= d <= N the index in device memory is exactly the index of the
// remaining text with first_line = F + d: the same records, val, postings (still global line
// numbers), text bytes, line starts and num_newlines that run_index(remaining_text, F + d) would
// have left, so index_resident() and every search_resident() answer field for field as a
// one-pass job over the remaining lines does.  Every list is non-decreasing in the line number,
// so what a word loses is a prefix of its list: nothing is renumbered and nothing is sorted
// (kernels/drop.hip); words whose lists empty out leave the dictionary.
//  * num_lines, num_tokens and num_unique are exact.  overflow_lines and truncated are exact
//    too: the dropped lines' share is counted on the device and subtracted.  max_key_len (the
//    statistic) is a maximum and cannot be subtracted: it stays as it was, "the longest the
//    index has held".
//  * d == 0 is a no-op that still reports the index's figures.  d == N leaves an empty index
//    whose first_line is F + N; append_index goes on from there (an empty resident text counts
//    as "ends in a newline").  A last line without its '\n' may be dropped with the rest.  Drops
//    and appends may follow each other in any order.
//  * Refused before anything is enqueued, the resident index intact and still searchable: no
//    resident index or a stale one; d > N.
//  * Any failure after the first kernel is enqueued leaves the index stale.
// Only counters cross PCIe (the byte offset of the cut among them).
struct IndexDrop {
  u64 dropped_lines = 0, dropped_tokens = 0;
  u64 dropped_words = 0;   // words whose list emptied
  u64 dropped_bytes = 0;   // text bytes removed
  u64 dropped_overflow_lines = 0, dropped_truncated = 0;
  u64 dropped_files = 0;   // non-empty segments that lay wholly inside the dropped lines ("corpus")
  u64 first_line = 0, num_lines = 0, num_tokens = 0, num_unique = 0;  // the resident index afterwards
  double drop_ms = 0;      // device time of the drop
  u64 store_bytes = 0;     // device bytes of the index store (both halves and the scratches)
};
// The host twin of the device drop: the index of x's text without its first `lines` lines, from
// the index alone, with merge_index's checks (keys strictly ascending, the counts adding up to
// the postings, every list non-decreasing).  An IndexResult holds no text, so the dropped lines'
// share of overflow_lines and truncated is the caller's to supply (a block's own run_index has
// them); max_key_len stays.  Throws when lines > x.words.num_lines.
//   trim_index(merge_index(a, b), a.words.num_lines, a.words.overflow_lines, a.words.truncated)
// equals b in entries, postings, first_line and every statistic but max_key_len.
IndexResult trim_index(const IndexResult& x, u64 lines, u64 dropped_overflow_lines = 0,
                       u64 dropped_truncated = 0);
// `in` cut into line-aligned blocks of at most block_bytes bytes, num_lines and first_line
// filled in; every block but the last ends in '\n', and a text that fits is one block.  A
// single line longer than block_bytes is an error (it names the CLI's --block-kb).
std::vector<TextInput> split_blocks(const TextInput& in, u64 block_bytes);

// ---- index search: all/any/phrase/near word queries over the inverted index ----
// A query is 1 to kSearchMaxTerms terms and a mode.  A term is a non-empty byte string
// without NUL, newline or a byte of the job's delimiter set; one longer than max_key_len is
// cut to its first max_key_len bytes, as the map cuts keys, and so matches the merged list
// of every long word with that prefix.  A term's lines are the distinct lines of its
// postings list (none when the word is absent).  `all` answers the intersection of the
// terms' lines (empty as soon as one term is absent), `any` their union; a term repeated
// inside a query changes nothing.  The answer is global line numbers, ascending, each once:
// a pure function of the index.  Each term also reports its word's count (0: absent).
//
// `phrase` answers the lines on which the terms occur as consecutive tokens, in order.
// A line's token sequence is exactly what the word job emits for it, in order: the job's
// delimiter set, a NUL ends the line's tokens, only the first emits_per_line tokens, each
// token cut to max_key_len bytes.  A line with tokens k_0 .. k_(n-1) matches the terms
// t_0 .. t_(m-1), each cut to max_key_len bytes, when some o exists with k_(o+j) == t_j
// for every j in [0, m).  Tokens past the emit cap do not exist for this purpose, a phrase
// never crosses a line end, and what stood between two consecutive tokens does not matter:
// any run of delimiters, of any length, counts.  Repeated terms are significant here:
// [bye, bye] matches only a line with two consecutive bye tokens.  A one-term phrase
// answers as `all` does, an absent term gives an empty answer, and long tokens that merge
// under truncation match as their merged key, the rule the index uses.  The answer and the
// per-term counts have the shape of the other modes'; repeated terms report the same count.
//
// `near` answers the lines on which the terms occur within W tokens of one another, in any
// order.  The window W (SearchQuery::within) is a u32 >= 1 given per query; W = 0, a `near`
// query without a window and a window on a query of another mode are refused.  A line's
// token sequence is exactly the phrase mode's: the job's delimiter set, a NUL ends the
// line's tokens, only the first emits_per_line tokens exist, each token cut to max_key_len
// bytes.  A line with tokens k_0 .. k_(n-1) matches when positions a <= b exist with
// b - a + 1 <= W such that every term is matched by at least one token k_i, a <= i <= b.
// Token matching is the phrase verification's: a plain term matches a token by equality of
// cut keys, a prefix term p when the token's cut key starts with p.  Order does not matter
// ([be, to] answers as [to, be]); a repeated term changes nothing (set semantics, as in
// `all`: [bye, bye] needs one bye); one token may satisfy several terms, which happens only
// with prefix terms ([Ham*, Hamlet] with W = 1 matches every line with the token Hamlet).
// A window never crosses a line end, an absent term gives an empty answer, a one-term query
// answers as `all` does, and so does every W >= emits_per_line (no line has more tokens):
// the engines take that shortcut and verify nothing.  term_counts, `merged` and the ranked
// score (tf over the whole line, from the postings -- not over the window) are `all`'s.
//
// Exclusion terms.  A query has 1 or more positive terms and 0 or more exclusion terms
// (SearchQuery::excluded: the last `excluded` entries of `terms`); together they number at
// most kSearchMaxTerms.  An exclusion term is validated, cut to max_key_len and, with
// wildcards, read as a prefix term exactly as a positive term is.
//   Excluded lines.  A term's lines are the distinct lines of its postings list, as for
//     `all`; a prefix term's list is its merged list.  A query's excluded lines are the union
//     of its exclusion terms' lines.  An absent exclusion term excludes nothing: it does not
//     empty the answer, unlike an absent positive term in `all`.
//   Matching set.  The matching set is what the mode answers for the positive terms alone,
//     minus the excluded lines.  The mode, the `near` window, the repetition rules and the
//     one-term shortcuts apply to the positive terms only: the `near` shortcut "W >=
//     emits_per_line answers as `all`" and the shortcut "one distinct term answers as `all`"
//     count distinct positive terms, and phrase and `near` verification sees only the positive
//     terms.  [alpha beta] not gamma as a phrase matches the line `alpha beta delta` and does
//     not match `alpha beta gamma`: the second line is excluded because it holds gamma
//     anywhere among its emitted tokens.
//   Pure function of the index.  Exclusion depends only on the index, so a token past the
//     emit cap excludes nothing: the rule every other mode follows.
//   Overlap with a positive term.  An exclusion term whose words equal or contain a positive
//     term's words empties `all`, `phrase` and `near`; in `any` it removes that term's lines
//     from the union.  This is legal, not an error.
//   Ranked.  `matches` counts the matching set after exclusion.  Exclusion terms take no part
//     in the score, in the "distinct present terms" or in the nesting rule: in Ham* not
//     Hamlet, Ham* still scores with its full merged count.  The bound score <= 32 *
//     emits_per_line is unchanged.
//   term_counts report every term, positive terms first and then the exclusion terms in the
//     order given; an exclusion term reports its word's count, or its merged count.
//   `merged`: the rule is unchanged and runs over all of the query's terms: the sum of the
//     counts over the query's terms that cover two or more words, a term whose words repeat
//     an earlier term's left out.  An exclusion prefix term covering two or more words is
//     therefore merged by the expand stage and counted; one covering a single word uses that
//     word's list in place.
//   Refused with a clear error: a query with no positive term, more than kSearchMaxTerms
//     terms in total, an invalid exclusion term, a lone `*` with wildcards.
//
// The device stage (kernels/search.hip; GpuWordCount::run_search / search_resident)
// answers batches of up to kSearchMaxQueries queries from the index in device memory:
// neither postings nor records cross PCIe.  A phrase or a `near` query takes its candidate
// lines from the `all` evaluation and verifies each against the text, which the engine
// keeps in device memory beside the index.  The host evaluation (search_index) takes any
// number of queries; for a phrase, or a `near` query of two or more terms, it needs the
// text too (the four-argument overload).
//
// ---- ranked search: the best K lines of every query, best first ----
// The matching set of a query is exactly what `all` / `any` / `phrase` / `near` answer.  Ranking
// never changes which lines match, only their order and how many are returned.
//   N            the index's postings.size() (= num_tokens, and val[n] on the device).
//   distinct present terms
//                the query's terms, each cut to max_key_len bytes; a term whose cut key
//                repeats an earlier one counts once (in `phrase` mode too, where repetition
//                matters for matching only); a term whose word is absent contributes nothing.
//   c_t          the term's word count (> 0 for a present term).
//   weight(t)    bit_length(N / c_t) = 32 - clz(N / c_t), integer division: in [1, 32]
//                because 1 <= c_t <= N < 2^32.  A rarer word weighs more.
//   tf(t, line)  how often `line` occurs in t's postings list (one posting per occurrence;
//                long tokens merged under truncation count together, as in the index).
//   score(query, line)
//                the sum over the distinct present terms of weight(t) * tf(t, line), a u32.
// Every matching line holds at least one present term in every mode, so it scores at least 1
// (a score of 0 for a hit is an internal error: the device counts it and the host throws).
// A line's tf values sum to at most emits_per_line, so score <= 32 * emits_per_line; a ranked
// search is refused when emits_per_line > kRankMaxEmits, so every accepted score is at most
// kRankScoreMax = 2^21 and fits a 22-bit field.  An unranked search knows no such limit.
// The answer of a query: `matches`, the number of matching lines (the unranked hit count),
// and the first min(K, matches) matching lines in the order (score descending, line
// ascending), each with its score.  The order is total, so the answer is unique.  K is one
// u32 >= 1 per batch; rank_k == 0 means the unranked answer.
//
// ---- prefix terms: `ham*` ----
// A term of a query may be a prefix term with prefix p (SearchQuery::prefix[t] != 0, terms[t]
// holding p without the star).  p is non-empty, validated exactly as a term is and cut to
// max_key_len bytes as a term is.  Its words are the index keys k with k[:len(p)] == p, a
// word equal to p among them: the keys are in unsigned-byte order, so they are one
// contiguous rank range [lo, hi), and their postings one contiguous range of the CSR.  Its
// list is the multiset union of those words' postings, non-decreasing; its count, as
// reported in term_counts, is the sum of their counts.  If no word matches, the term is
// absent.  If len(p) == max_key_len (after the cut), it is exactly the plain term p.
// In `all`, `any` and the candidate stage of `phrase` and `near`, a prefix term behaves as a
// word with that list.  In `phrase` and `near` verification a token matches a prefix term
// when the token's key (cut to max_key_len) starts with p; a token shorter than p does not.
// Ranked: a prefix term's c_t is its merged count (the weight still bit_length(N / c_t), in
// [1, 32]) and its tf the line's multiplicity in the merged list.  Prefix ranges and single
// words form a laminar family: two terms' key ranges are nested or disjoint.  A present
// term whose key range lies inside the range of another present term of the same query
// contributes nothing to the score; of equal ranges the first occurrence counts (for plain
// terms this is "a repeated key counts once").  The remaining terms have disjoint ranges,
// so a line's tf values still sum to at most emits_per_line and every bound above holds
// unchanged.  Matching is not affected by this rule.
// The device merges the list of a prefix term that covers two or more words (one radix sort
// of all such lists of the batch, kernels.hpp "search.hip"); SearchResult::merged is the
// number of list elements it merged: over the batch's prefix terms that cover two or more
// words, a term whose range repeats an earlier term's of its query left out, the sum of
// their counts.  A term covering one word uses that word's list in place.
// `*` is no delimiter: `ham*` is a legal literal token, and stays one unless the caller
// asks for wildcards (make_search_query).
//
// ---- pattern terms: `*ing`, `h?mlet`, and ignore_case ----
// A term may be a pattern term (SearchQuery::pattern[t] != 0, terms[t] holding the pattern as
// asked, runs of `*` collapsed to one).  make_search_query's `glob` makes them: after the
// collapse a term without `*` or `?` is a plain term, `p*` with p non-empty and free of
// metacharacters is the prefix term of the section above (its cut rule included: glob is a
// superset of wildcard, and both together are glob), and anything else that holds a `*` or a
// `?` is a pattern term.  There is no escape character.  A pattern's bytes other than `*` and
// `?` are validated as a term's are; a pattern longer than max_key_len bytes (a pattern is
// never cut) and one with no byte other than `*` are refused.  `???` is legal.
//   Words.  A pattern term's words are the index keys k, as the index holds them (cut to
//     max_key_len, their length the bytes before the NUL padding), that the pattern matches
//     as a whole: `*` matches any run of bytes, the empty run included; `?` exactly one byte
//     and never the padding (`ab?` does not match the key `ab`); every other byte itself
//     (device/glob.hpp: the one matcher both engines use).  The words are a scattered set of
//     ranks, not a range.  The term's list is the multiset union of its words' postings, non-
//     decreasing; its count the sum of their counts; without a word it is absent.
//   ignore_case is a property of a whole batch.  Every term of the batch -- positive or
//     exclusion; plain, prefix or pattern -- is cut exactly as without it and then evaluated as
//     a pattern term whose bytes A-Z and a-z match either case: plain `hamlet` is the pattern
//     `hamlet` (a `*` or `?` in it stays literal), prefix `ham*` the pattern `ham*`.  Only
//     ASCII letters fold: `@`, `[`, `` ` ``, `{` and every byte of 0x80 or above match only
//     themselves.
//   Modes.  In `all`, `any`, exclusion and the candidate stage of `phrase` and `near` a pattern
//     term is a word with its list.  In `phrase` and `near` verification a token matches a
//     pattern term when its cut key matches the pattern under the same rule and the same fold.
//     Absent-term rules, one-term shortcuts, the emit cap and the `near` window are unchanged.
//   Identity.  Two pattern terms of a query are the same term when their pattern bytes (and
//     which of them are metacharacters) are equal -- under ignore_case: equal after lower-casing
//     ASCII.  The later one repeats the earlier one: it reports the same count, is not merged
//     again and scores once.  A pattern term is never the same as a plain or prefix term, even
//     when their word sets coincide; it is never inside another term's range and no term is
//     inside it: the laminar-family rule applies to plain and prefix terms among themselves.
//   Ranked.  weight and tf are a prefix term's: c_t is the term's count, tf the line's
//     multiplicity in its list.  Lists of pattern terms may overlap, so one token may count for
//     up to eight terms: a score is at most 32 * emits_per_line * 8.  A ranked batch that holds
//     a pattern term (every batch under ignore_case) is refused when emits_per_line >
//     kRankMaxEmits / 8, so the 22-bit score field still suffices; the device's `unscored`
//     bound and validate_search's upper bound are 32 * emits_per_line * 8 for such a batch and
//     unchanged for every other.
//   `merged` adds the count of every pattern term that covers two or more words and repeats no
//     earlier term of its query; one with exactly one word uses that word's list in place.
//   `any` bound.  Overlapping lists can push a query's `any` bound past 2^32: the lookup sums
//     in u64, counts the overflow and the host throws.
//   term_counts keep their order, and format_search_output prints a pattern term as asked.
// The device finds a pattern term's words by a scan of the dictionary (kernels.hpp
// "search.hip": match, scatter): (pattern slots) x (dictionary words) matcher calls per batch,
// twice for the slots that cover two or more words.
//
// ---- fuzzy terms: `Hamlet~1`, `quene~2` ----
// A term may be a fuzzy term of a word w with a budget d (SearchQuery::fuzzy[t] == d, 1 or 2,
// terms[t] holding w without the suffix).  make_search_query's `fuzzy` makes them, and only it:
// without it `Hamlet~1` is the literal word it has always been.
//   Syntax.  With `fuzzy`, a term t of three or more bytes whose last byte is a decimal digit
//     and whose last byte but one is `~` is the fuzzy term of w = t without its last two bytes
//     and d = the digit.  d must be 1 or 2: any other digit is refused.  A `~` anywhere else is
//     a literal byte of its word: with no digit behind it, with two digits behind it, or with
//     `~1` in the middle of a word.  This reading comes before the wildcard and glob reading of
//     the term.
//   The word.  w is validated byte for byte as a term is: no NUL, no newline, no delimiter.  w
//     is never cut: len(w) > max_key_len is refused, as for a pattern.  w must be longer than
//     its budget: len(w) <= d is refused (`a~1` would match every word of one or two bytes).
//     With glob or wildcard also on, a w that holds `*` or `?` is refused: a term is fuzzy or a
//     pattern, never both.  `fuzzy` does not imply wildcard or glob, and combines with both and
//     with ignore_case.
//   Words.  A fuzzy term's words are the index keys k, as the index holds them (cut to
//     max_key_len, their length the bytes before the NUL padding), with lev(w, k) <= d.  lev is
//     the Levenshtein distance over bytes: one insertion, deletion or substitution of a byte
//     costs 1; there is no transposition and no UTF-8 awareness.  Two bytes are equal as the
//     pattern matcher's literal bytes are (glob_byte_eq): under the batch's ignore_case ASCII
//     letters match either case, and nothing else folds.  A long word cut to max_key_len
//     matches as its merged key, the rule the index uses everywhere.  (device/fuzzy.hpp: the
//     one matcher both engines use.)
//   Everything else is a pattern term's rule with this matcher in place of the pattern's.  The
//     term's list is the multiset union of its words' postings, its count the sum of their
//     counts, and without a word it is absent.  In `all`, `any`, exclusion and the candidate
//     stage it is a word with that list; in `phrase` and `near` verification and in show spans a
//     token matches when its cut key is within d of w under the same fold.  search_has_patterns
//     is true for a batch that holds a fuzzy term: the ranked bound is 32 * emits_per_line * 8,
//     and a ranked batch is refused when emits_per_line > kRankMaxEmits / 8.  `merged` counts a
//     fuzzy term that covers two or more words and repeats no earlier term of its query; one
//     with exactly one word uses that list in place.  The `any`-bound overflow rule holds.
//   Identity.  Two fuzzy terms of a query are the same term when their w bytes and their budget
//     are equal -- under ignore_case: the bytes after lower-casing ASCII.  `ham~1` and `ham~2`
//     are different terms.  A fuzzy term is never the same as a plain, prefix or pattern term,
//     and takes no part in the laminar nesting rule.
//   term_counts keep their order, and format_search_output prints the term as asked: `Hamlet~1`.
// The device finds a fuzzy term's words by the pattern terms' scan of the dictionary, and a
// batch that holds one runs kernels compiled with both matchers (kernels.hpp "fuzzy.hip").
//
// ---- regex terms: `/\[?Hamlet[!?\]]?/`, `/(king|queen)[!?]?/` ----
// A term may be a regex term (SearchQuery::regex[t] != 0, terms[t] holding the source without
// the slashes).  make_search_query's and make_search_expr's `regex` makes them, and only it:
// without it `/x/` is the literal word it has always been.
//   Reading.  With `regex`, a term that starts with `/` is a regex term.  It must be at least
//     three bytes long and end in a `/` that is not escaped; its source is what stands between
//     the slashes, and `\/` in the source is a literal slash.  A term that starts with `/` and
//     is not of that shape (`/`, `//`, `/ab`) is refused.  This reading comes before the fuzzy,
//     wildcard and glob readings, and nothing inside the slashes is read by them.  `regex`
//     implies none of the other switches and combines with all of them, ignore_case included.
//   Syntax.  Bytes, not characters: no UTF-8 awareness.  A literal byte.  `\` followed by a byte
//     that is no ASCII letter or digit: that byte, literally; `\` followed by a letter or digit
//     is refused (reserved: there is no `\d` or `\w`).  `.`: any one byte.  `[...]` and `[^...]`:
//     a class whose members are single bytes or ranges `a-z`; `\` escapes inside it and `]` must
//     be escaped; `-` first or last is literal; `^` is special only as the first byte; a range
//     with lo > hi, an empty class and an unterminated class are refused.  `( ... )` groups and
//     `|` alternates; `*`, `+`, `?` repeat the atom before them.  An empty branch or group
//     matches the empty string: `(a|)` and `()` are legal.  Refused, with an error that names the
//     cause: the empty source; a quantifier with nothing to repeat or directly after another
//     quantifier (`a**`, `a*?`, `(?`); an unescaped `{`, `}`, `^` or `$` outside a class;
//     unbalanced parentheses; a NUL or a newline anywhere in the source; nesting deeper than
//     kRegexMaxDepth = 32; a source longer than kRegexMaxSource = 128 bytes; more than
//     kRegexMaxPos = 32 positions, a position being one literal, one `.` or one class.  A byte
//     of the job's delimiter set in the source is legal (`.`, `(`, `)` and `-` are default
//     delimiters and syntax here): a literal delimiter simply matches no key.  A regex is never
//     cut to max_key_len.
//   Words.  A regex term's words are the index keys whose whole key the expression matches --
//     keys as the index holds them (cut to max_key_len, their length the bytes before the NUL
//     padding), the match anchored at both ends.  `.` and a negated class never match the
//     padding: `/ab./` does not match the key `ab`.  A long word cut to max_key_len matches as
//     its merged key, as everywhere.
//   ignore_case.  The fold is the batch's.  A position's byte set, taken before a class's
//     negation, is closed under the ASCII letter case swap and then negated: `/[^a]/` matches
//     neither `a` nor `A`.  Only A-Z and a-z fold.
//   Everything else is a pattern term's rule with this matcher (device/regex.hpp: the one
//     matcher both engines use, over the program compile_regex builds).  The list is the
//     multiset union of the words' postings, the count the sum of their counts; without a word
//     the term is absent; one word uses its list in place, two or more are merged and counted in
//     `merged`.  In `all`, `any`, `expr`, exclusion and the candidate stage it is a word with
//     that list; in `phrase` and `near` verification and in show spans a token matches when its
//     cut key matches the regex under the batch's fold.  search_has_patterns is true for a batch
//     that holds one (the 32 * emits_per_line * 8 score bound, the kRankMaxEmits / 8 refusal),
//     and the `any`-bound overflow rule holds.
//   Identity.  Two regex terms of a query are the same term when their source bytes are equal,
//     byte for byte, also under ignore_case.  A regex term is never the same as a term of
//     another kind, and takes no part in the nesting rule.
//   term_counts keep their order, and format_search_output prints the term as asked, slashes
//     included.
//   `expr` mode.  With `regex`, a token of an expression that begins with `/` runs to the next
//     unescaped `/`: blanks and parentheses inside belong to it.  The closing slash must be
//     followed by a blank, a parenthesis or the end.
// The device finds a regex term's words by the pattern terms' scan of the dictionary with the
// compiled programs in a device table, and a batch that holds one runs kernels compiled with all
// three matchers (kernels.hpp "regex.hip").
//
// ---- boolean expressions: `( to AND be ) OR ( Ham* AND NOT Hamlet )` ----
// A fifth mode, `expr` (SearchMode::kExpr; make_search_expr makes the query), answers a Boolean
// expression over up to kSearchMaxTerms terms.
//   Syntax.  An expression is a byte string.  Blanks and tabs separate tokens; `(` and `)` are
//     always grouping tokens by themselves, wherever they stand (`(to AND be)`).  The tokens
//     `AND`, `OR` and `NOT`, exactly these upper-case bytes, are operators; every other token is
//     a term.  Precedence: NOT > AND > OR; AND and OR associate to the left.  Two operands side by
//     side are joined by an implicit AND: `to be` is `to AND be`.  `and`, `or` and `not` in lower
//     case are ordinary words; the literal word `AND` cannot be asked for in this mode.
//   Terms.  A term is read exactly as a term of make_search_query is, under the same wildcard,
//     glob and fuzzy settings (and the batch's ignore_case) and with their errors, and is cut to
//     max_key_len at evaluation as every term is.  A term that holds a NUL, a newline or a byte
//     of the job's delimiter set is refused.  Two operands are the same term when they read to
//     the same bytes and the same kind (plain, prefix, pattern, fuzzy with its budget).  A query
//     has 1 to kSearchMaxTerms distinct terms, numbered in order of first occurrence;
//     SearchQuery::terms, prefix, pattern and fuzzy hold them as for any query, excluded == 0.
//     SearchQuery::expr is the text as asked, runs of blanks and tabs collapsed to one space and
//     the ends trimmed; SearchQuery::truth is the expression's truth table, 8 x u32: bit m (bit
//     m % 32 of word m / 32) is its value when exactly the terms in mask m hold.
//   Meaning.  A term's lines are the distinct lines of its list (a prefix, pattern or fuzzy term:
//     of its merged list).  An absent term has no lines: its bit is never set, and it does not
//     empty the answer.  A line's mask has bit t set when the line is among term t's lines, and
//     the line matches when truth[mask] is set.  The answer is a pure function of the index:
//     ascending global line numbers, each once.  term_counts are in term order; `merged` is the
//     existing rule over the query's terms.
//   Refused, with an error that names the cause: an empty expression, unbalanced parentheses,
//     `()`, a dangling operator (`a AND`, `OR b`, `NOT`), more than kSearchMaxTerms distinct
//     terms, parentheses nested deeper than kExprMaxDepth (the parser recurses once per open
//     parenthesis and never deeper; runs of NOT are folded in a loop), and an expression with
//     truth[0] set -- one that is true of a line holding none of its words, such as `NOT a` or
//     `a OR NOT b`: the index cannot enumerate such lines.  `exclude` and `within` on an `expr`
//     query are refused: use NOT.  `a AND NOT a` is legal and answers nothing.
//   Ranked.  The matching set is as above.  The score is `any`'s: the sum over the distinct
//     present terms of the expression of weight(t) * tf(t, line), whether or not a term stands
//     under a NOT, with the nesting rule of prefix terms unchanged (and a pattern identical to an
//     earlier one under ignore_case counted once).  Every match holds at least one present term
//     (truth[0] is clear), so it scores at least 1; the score bound and the emits_per_line limits
//     are unchanged.
//   Show and mark work as for `any`: every emitted token that matches one of the expression's
//     terms is a span, under a NOT or not, and mask bit t names term t.
//   Output.  The query's result line prints `expr` where the other modes print the joined terms.
// The walked set.  The device does not walk the union of all terms' lists (`to AND NOT the` would
// read the's list to find lines that all come from to's) but the lists of a set S of terms.
// Let P be the present terms.  S covers when every mask m that is a subset of P and has truth[m]
// set meets S: then every matching line lies in a list of S.  S is chosen greedily from the list
// lengths: start with S = P; take the terms in order of list length descending, of equal lengths
// the higher term number first; drop a term from S when the rest still covers.  If no m inside P
// has truth[m] set, S is empty and the query walks nothing.  SearchResult::walked is the number
// of list elements the device's hit stage walked for the batch: the sum over its queries of
// their bounds (`all`: the driver's list, `any`: the distinct lists, `expr`: the lists of S).  A
// host evaluation reports 0.
// The device stage (kernels/expr.hip) looks an `expr` query up as `any` over all its terms, plans
// S per query, walks S's lists and decides every first occurrence of a line by one lookup in the
// 256-bit table: no expression tree is interpreted in a kernel.
// ---- show: the returned lines' text and match spans ----
// A search job may ask for show = N, a u32 with 1 <= N <= kShowMaxBytes = 65536; show == 0,
// the default, is the answer described above, bit for bit.  With show = N every entry i of
// `lines` -- in result order: unranked, per query ascending; ranked, the min(K, matches)
// winners in rank order -- also gets:
//   text   the line's bytes from its start to its end, cut to the first N bytes.  The end is
//     the '\n', the end of the input, or a NUL: exactly where the tokenisers stop.  cut_lines
//     counts the entries whose line was longer than N.
//   spans  one (start, len, mask) triple of u32 for every emitted token of the line (ordinal <
//     emits_per_line) that matches at least one positive term of that entry's query, in token
//     order.  start is the byte offset from the line's start; len the token's full length up to
//     the next delimiter or the line's end, cut neither to max_key_len nor to N; mask bit j is
//     set when the token matches positive term j.  A token matches a term as the phrase and
//     `near` verification match them: equality of cut keys, a prefix term's bytes, a pattern
//     term's matcher, under the batch's fold with ignore_case.  A term that repeats an earlier
//     one sets its own bit too.  Exclusion terms never produce a span.  The rule is the same in
//     every mode: in `phrase` and `near` every token that matches a term is a span, not only
//     those inside an occurrence or a window.  A token past the emit cap produces nothing, as
//     everywhere else.
// The same line returned for two queries is two entries, each with its own spans.  Entry i's
// text is text[text_off[i] .. text_off[i + 1]), its triples spans[3 * span_off[i] .. 3 *
// span_off[i + 1]).  Refused with a clear error: N out of range; a job whose text window holds
// 2^32 bytes or more (a span's start is a u32); on the device, a payload (text, spans and both
// offset arrays) that does not fit the free device memory or the pinned buffer
// (kShowMaxPayload) -- the index stays resident behind a refused show.
// The device stage (kernels/show.hip) runs behind the search stage on the resident text, line
// starts, keys and returned lines: the text itself never crosses PCIe, only the shown bytes and
// spans do (wire_bytes counts them).  The host evaluation needs the text: the four-argument
// search_index.
// ---- tally: the words of the returned lines ----
// A search job may ask for tally = K, a u32 with 1 <= K <= kTopKMax; tally == 0, the default, is
// the answer described above, bit for bit, and launches nothing new.  With tally = K every query
// q of the batch also gets the counts of the index's words over its returned lines:
//   returned lines  exactly the entries show would print: unranked, the whole matching set;
//     ranked, the min(rank_k, matches) winners.  The same line returned for two queries counts
//     for each of them.
//   count(q, w)  the number of postings of word w whose line is a returned line of q: a pure
//     function of the index and the returned lines.  A token past the emit cap does not exist,
//     long tokens merged under truncation count as their merged key, a word twice on a line
//     counts twice.  Equivalently: the word job's count of w over the returned lines alone, under
//     the job's own delimiters, emit cap and key cut.
//   The mode, the window, exclusion terms, prefix, pattern, fuzzy and regex terms and
//   ignore_case decide which lines are returned, and nothing else: keys are counted as the index
//   holds them (`To` and `to` are two words even under ignore_case), the query's own words like
//   any other.
// Per query: tally_words[q], the words with count > 0; tally_tokens[q], the sum of all counts
// (the emitted tokens of the returned lines); and the first min(K, tally_words[q]) words in the
// order count descending, key ascending in unsigned-byte order (the top-K order above: total),
// each with its key and u64 count.  A word with count 0 is never returned; a query that returns
// no line gets 0, 0 and no word.  `tallied` is the sum of tally_tokens over the batch: the pair
// words the device stage sorts (0 for the host evaluation, as merged and walked are).
// Refused with a clear error: K out of range; tally without a search; on the device, a
// workspace that does not fit the free device memory (the index stays resident behind the
// refusal, as behind a refused show) and a batch whose rank key does not fit: with r =
// bit_length(n - 1) rank bits for n index words and c = bit_length(T) count bits for T pair
// words, T >= 2^32 or c + r > 54 (the key is query << 54 | (2^c - 1 - count) << r | rank).
// The device stage (kernels/tally.hip) re-tokenises the returned lines from the resident text;
// the host evaluation walks the postings word by word against a bitmap of each query's returned
// lines and needs no text.  Only the winners' records, three per-query arrays and the counters
// cross PCIe (wire_bytes counts them).
struct TallyKeySplit {
  u32 r = 0, c = 0;
  u64 cmask = 0;
};
// The split for n index words and `tokens` pair words; throws as described above.
TallyKeySplit tally_key_split(u64 n, u64 tokens);
// File sets.  SearchQuery::files is a sorted list of distinct segment ids ("corpus" above);
// empty means every file.  The matching set of a query is what its mode answers, after
// exclusion, intersected with the lines whose segment's id is in the set -- for all / any /
// phrase / near / expr alike.  An id that is not resident selects nothing and is no error: it
// may never have been begun, or it may have been dropped.  The set selects lines only: N and
// every count of a ranked score stay those of the whole resident index, so the ranked answer
// under a set is the unrestricted ranking filtered to the set and cut to K.  matches, the K
// winners, show and tally all see the restricted set.  Refused: ids not strictly ascending.
// On the device a batch with at least one non-empty set runs the restrict stage (kernels.hpp
// "corpus.hip") between the hit / verify kernels and the sort; any other batch enqueues what it
// always did.
// Answers by file.  A batch may ask for by_file = kByFile: beside `lines` it returns line_file
// and line_local, the segment id and file-local number of every returned line (ranked: in rank
// order), and a CSR -- per query the files with at least one returned line, ids ascending, and
// their counts, which add up to the query's returned lines (unranked: every match; ranked: the
// min(K, matches) winners, the rule tally follows).  kByFileCount is `grep -c`: only the CSR,
// `matches` and the counters cross PCIe; `lines` and `offsets` stay empty (offsets all 0) and
// the lines stay on the device.  It is refused with rank, show or tally.  The device stage
// (kernels.hpp "corpus.hip") stands behind emit / top; wire_bytes counts exactly what is copied.
constexpr u32 kByFileNone = 0, kByFile = 1, kByFileCount = 2;
constexpr u32 kShowMaxBytes = 65536;
constexpr u64 kShowMaxPayload = 4ull << 30;  // bytes of one batch's show payload on the device
constexpr u32 kSearchMaxQueries = 1024;
constexpr u32 kSearchMaxTerms = 8;
constexpr u64 kRankMaxEmits = 65536;
constexpr u32 kRankScoreMax = 32u * (u32)kRankMaxEmits;  // 2^21
constexpr u64 kSearchMaxWithin = 0xffffffffull;  // a `near` window: 1 <= W <= 2^32 - 1
constexpr int kExprMaxDepth = 64;  // "boolean expressions": open parentheses around one operand
constexpr int kExprTruthWords = 8;  // the 256-bit truth table of kSearchMaxTerms terms
constexpr int kRegexMaxDepth = 32;     // "regex terms": open parentheses around one atom
constexpr size_t kRegexMaxSource = 128;  // ... the bytes of a source
enum class SearchMode { kAll, kAny, kPhrase, kNear, kExpr };
struct SearchQuery {
  std::vector<std::string> terms;
  SearchMode mode = SearchMode::kAll;
  u64 within = 0;  // kNear: the window W in tokens, 1 .. kSearchMaxWithin; other modes: 0
  std::vector<u8> prefix;  // empty: no prefix term; else parallel to terms, != 0: a prefix term
  u32 excluded = 0;  // the last `excluded` entries of terms are exclusion terms ("not")
  std::vector<u8> pattern;  // empty: no pattern term; else parallel to terms, != 0: a pattern term
  std::vector<u8> fuzzy;  // empty: no fuzzy term; else parallel to terms, 1 or 2: a fuzzy term's
                          // budget (terms[t]: its word, without the `~d`), 0: none
  std::vector<u8> regex;  // empty: no regex term; else parallel to terms, != 0: a regex term
                          // (terms[t]: its source, without the slashes)
  std::string expr;       // kExpr: the expression as asked, blanks collapsed ("boolean expressions")
  std::array<u32, kExprTruthWords> truth{};  // kExpr: bit m: the value when exactly mask m holds
  std::vector<u32> files;  // "file sets" above: segment ids, strictly ascending; empty: every file
  bool truth_at(u32 m) const { return (truth[(m >> 5) & 7u] >> (m & 31u)) & 1u; }
  bool is_prefix(size_t t) const { return t < prefix.size() && prefix[t] != 0; }
  u32 fuzzy_budget(size_t t) const { return t < fuzzy.size() ? fuzzy[t] : 0u; }
  bool is_pattern(size_t t) const { return t < pattern.size() && pattern[t] != 0; }
  bool is_regex(size_t t) const { return t < regex.size() && regex[t] != 0; }
  // the positive terms: terms[0 .. positives())
  size_t positives() const { return excluded < terms.size() ? terms.size() - excluded : 0; }
};
struct SearchResult {
  std::vector<SearchQuery> queries;  // as asked (terms uncut)
  std::vector<u64> offsets;          // [queries + 1]: query i's lines are lines[offsets[i] .. offsets[i+1])
  std::vector<u32> lines;            // global line numbers, per query strictly ascending
                                     // (ranked: per query in rank order)
  std::vector<u64> term_counts;      // [queries * kSearchMaxTerms]: term t of query i at i * 8 + t
  u64 rank_k = 0;                    // 0: unranked
  std::vector<u32> scores;           // ranked: parallel to lines; unranked: empty
  std::vector<u64> matches;          // [queries] matching lines (unranked: the hit counts)
  u64 emits_per_line = 0;            // the job's (a ranked score is at most 32 * this)
  u64 merged = 0;                    // list elements the device merged for prefix terms (0:
                                     // none, or the host evaluation)
  u64 walked = 0;                    // list elements the device's hit stage walked: the sum of
                                     // the queries' bounds (0: the host evaluation)
  bool ignore_case = false;          // the batch was evaluated with ignore_case
  u64 first_line = 0;
  // the word job's statistics, as in TopResult
  u64 num_lines = 0;
  u64 num_tokens = 0;
  u64 num_unique = 0;
  u64 overflow_lines = 0;
  u64 truncated = 0;
  u64 max_key_len = 0;
  StageTimes times;
  double index_ms = 0;   // device time of the index stage (0: built on the host, or resident)
  double search_ms = 0;  // device time of the search stage (host evaluation: its wall time)
  u64 wire_bytes = 0;    // bytes the device wrote to host memory for the result
  // "show" above (show_bytes == 0: none of these is filled)
  u32 show_bytes = 0;          // N
  std::string text;            // the entries' shown bytes, one after the other
  std::vector<u64> text_off;   // [entries + 1]
  std::vector<u32> spans;      // (start, len, mask) triples
  std::vector<u64> span_off;   // [entries + 1], in triples
  u64 cut_lines = 0;           // entries whose line was longer than N
  double show_ms = 0;  // device time of the show stage (host evaluation: its wall time)
  // "tally" above (tally_k == 0: none of these is filled)
  u64 tally_k = 0;                     // K
  std::vector<u64> tally_off;          // [queries + 1]: query i's words, [tally_off[i], tally_off[i+1])
  std::vector<PackedKey> tally_keys;   // count descending, key ascending per query
  std::vector<u64> tally_counts;       // parallel to tally_keys
  std::vector<u64> tally_words;        // [queries] words with count > 0
  std::vector<u64> tally_tokens;       // [queries] the sum of all counts
  u64 tallied = 0;                     // pair words the device stage sorted (0: host evaluation)
  double tally_ms = 0;  // device time of the tally stage (host evaluation: its wall time)
  // "file sets" (engine.hpp): the table the batch was answered under (empty: one segment
  // (0, first_line, 0)) and the pair words the device's restrict stage removed (0: no file set
  // in the batch, or the host evaluation)
  std::vector<IndexSegment> segments;
  u64 restricted = 0;
  // "answers by file" (by_file == kByFileNone: none of these is filled)
  u32 by_file = 0;
  std::vector<u32> line_file;    // parallel to lines: the line's segment id (count only: empty)
  std::vector<u32> line_local;   // parallel to lines: its file-local number (count only: empty)
  std::vector<u64> file_off;     // [queries + 1]: query i's files, [file_off[i], file_off[i+1])
  std::vector<u32> file_ids;     // ascending per query: the files with a returned line
  std::vector<u32> file_counts;  // parallel to file_ids: their returned lines
  double by_file_ms = 0;  // device time of the by-file stage (host evaluation: 0)
  u64 hits() const { return lines.size(); }
};
// A term's key: its first min(size, cfg.max_key_len) bytes, packed as the map packs keys.
PackedKey search_term_key(const std::string& term, const JobConfig& cfg);
// Is term t of q a prefix term after the cut?  (A prefix of max_key_len bytes or more is
// exactly the plain term.)
inline bool search_term_prefix(const SearchQuery& q, size_t t, const JobConfig& cfg) {
  return q.is_prefix(t) && q.terms[t].size() < (size_t)cfg.max_key_len;
}
// The query of user terms.  wildcard: a term that ends in `*` and is longer than one byte
// becomes a prefix term of what precedes the star; a lone `*` is an error; a `*` anywhere
// else is literal.  Without wildcard every term is literal.
// within: the window of a `near` query (0: none).  exclude: the query's exclusion terms, read
// as `terms` are and appended behind them.  glob: "pattern terms" above (runs of `*` collapse;
// a lone star, or a run of them, is an error); with glob, wildcard changes nothing.
// fuzzy: "fuzzy terms" above (a trailing `~1` or `~2` makes a fuzzy term, read before the
// wildcard and glob reading; another digit, a word no longer than its budget and -- with
// wildcard or glob -- a word that holds `*` or `?` are errors).
// regex: "regex terms" above (a term that starts with `/` is `/source/`, read before every other
// reading; a malformed term and a source compile_regex refuses are errors).
SearchQuery make_search_query(const std::vector<std::string>& terms, SearchMode mode,
                              bool wildcard, u64 within = 0,
                              const std::vector<std::string>& exclude = {}, bool glob = false,
                              bool fuzzy = false, bool regex = false);
// The `expr` query of an expression ("boolean expressions" above): the parser, the terms'
// identification and the truth table.  Every term is read by make_search_query's rules under
// wildcard, glob and fuzzy, and validated for cfg (check_search_queries).  Throws with the cause
// for every refusal listed there.
// regex: a token that begins with `/` runs to the next unescaped `/` ("regex terms").
SearchQuery make_search_expr(const std::string& expr, const JobConfig& cfg, bool wildcard = false,
                             bool glob = false, bool fuzzy = false, bool regex = false);
// A regex term's compiled program ("regex terms"; the layout: device/regex.hpp, kRegexWords u32
// words): the Glushkov position automaton of `source` -- first, last, nullable, follow[32] and
// the byte table B[256] with the fold compiled in.  Throws with the cause for every refusal
// listed there.
std::vector<u32> compile_regex(const std::string& source, bool ignore_case);
// A term as the pattern it is evaluated as: the packed bytes (kv.hpp) and the map of its
// metacharacters (device/glob.hpp) -- a fuzzy term: its word's bytes and kFuzzyMeta | its
// budget as the device's meta word (device/fuzzy.hpp).
// The host reads the kind from fields of its own, never from a bit of `meta`: a pattern of 31
// bytes uses every bit of its map below bit 31, and a star behind 31 cut bytes would be bit 31
// itself.  `budget` != 0: a fuzzy term, matched by fuzzy_match.  `regex`: a regex term -- no
// bytes, meta 0, `rx` its compiled program (device/regex.hpp) and `src` its source, which is its
// identity.
struct SearchPattern {
  PackedKey p;
  u32 meta = 0;
  u32 budget = 0;
  bool regex = false;
  std::vector<u32> rx;
  std::string src;
  // the same term, as the identity rules say
  bool same(const SearchPattern& o) const {
    return regex == o.regex && budget == o.budget && meta == o.meta &&
           key_compare(p.w, o.p.w) == 0 && src == o.src;
  }
  // does the key (an index key, a token's cut key) match?
  bool matches(const u64* key, bool fold) const;
};
// Is term t of q evaluated as a pattern term -- a pattern term, a fuzzy term, or any term under
// ignore_case?  If so *out (when given) is its pattern: a pattern term's bytes as asked, a
// prefix term's cut prefix and a star, a plain term's cut bytes, all literal; under ignore_case
// with the ASCII letters lower-cased (two terms are the same term when their patterns are
// equal).
bool search_term_pattern(const SearchQuery& q, size_t t, const JobConfig& cfg, bool ignore_case,
                         SearchPattern* out = nullptr);
// Does a batch of these queries hold a term that is evaluated as a pattern term?  (A fuzzy
// term is.)
bool search_has_patterns(const std::vector<SearchQuery>& queries, bool ignore_case);
// Does it hold a fuzzy term?
bool search_has_fuzzy(const std::vector<SearchQuery>& queries);
// Does it hold a regex term?
bool search_has_regex(const std::vector<SearchQuery>& queries);
// Throws unless every query has 1..kSearchMaxTerms valid terms for cfg's delimiter set, at
// least one of them positive (and `prefix` empty or as long as `terms`), a `near` query a
// window in [1, kSearchMaxWithin] and every other query none (within == 0).  An `expr` query:
// no exclusion term, no window, and truth[0] clear.
void check_search_queries(const std::vector<SearchQuery>& queries, const JobConfig& cfg);
// Throws when the `elements` list elements a device batch's prefix terms merge
// (SearchResult::merged) do not fit the merge's 32-bit element counter.
void check_search_merge(u64 queries, u64 elements);
// Throws unless rank_k is 0 (unranked) or a u32 >= 1 with cfg.emits_per_line <= kRankMaxEmits
// (patterns: the batch holds a pattern term -- kRankMaxEmits / kSearchMaxTerms).
void check_search_rank(u64 rank_k, const JobConfig& cfg, bool patterns = false);
// Throws unless show is 0 (no show) or 1 <= show <= kShowMaxBytes and the window holds fewer
// than 2^32 bytes ("show" above).
void check_search_show(u64 show, u64 text_bytes);
// Throws unless tally is 0 (no tally) or 1 <= tally <= kTopKMax ("tally" above).
void check_search_tally(u64 tally);
// Throws unless by_file is kByFileNone, kByFile or kByFileCount, and kByFileCount stands without
// rank, show and tally ("answers by file" above).
void check_search_by_file(u32 by_file, u64 rank_k, u64 show, u64 tally);
// The host evaluation over an index result, any number of queries (cfg: the index job's
// delimiters and max_key_len).  Throws for a phrase query and for a `near` query of two or
// more terms: the index holds no positions, so they need the text -- the four-argument
// overload (what counts are the positive terms).
// rank_k != 0 ranks every query (scores come from the postings alone).
// ignore_case: "pattern terms" above.  Pattern terms' words come from a scan of the entries
// with the shared matcher.
// show != 0 is refused: the shown lines come from the text (the four-argument overload).
// tally = K: "tally" above, answered here too -- the rule needs no text.
SearchResult search_index(const IndexResult& x, const std::vector<SearchQuery>& queries,
                          const JobConfig& cfg, u64 rank_k = 0, bool ignore_case = false,
                          u64 show = 0, u64 tally = 0, u32 by_file = 0);
// The same with the text the index was built from (the same window: text.first_line ==
// x.first_line; cfg also gives emits_per_line): a phrase's or a `near` query's candidates
// come from the `all` evaluation and are verified by tokenising their lines with the CPU
// engine's tokeniser.  show = N: "show" above, from the same tokeniser and the shared matcher.
SearchResult search_index(const IndexResult& x, const TextInput& text,
                          const std::vector<SearchQuery>& queries, const JobConfig& cfg,
                          u64 rank_k = 0, bool ignore_case = false, u64 show = 0,
                          u64 tally = 0, u32 by_file = 0);
// LOCUST_CHECK invariants of a search result: offsets monotone from 0 to lines.size(), every
// line inside [first_line, first_line + num_lines), one `matches` per query.  Unranked: every
// query's lines strictly ascending, matches == the hit counts, no scores.  Ranked: one score
// per line, each in [1, 32 * emits_per_line] (a batch with a pattern term: times 8), per query
// non-increasing with equal scores on ascending lines, and at most min(rank_k, matches) lines
// per query.  With show: both offset arrays monotone from 0 to their array's size, every text
// length <= N, and per entry the spans strictly ascending and non-overlapping, start + len
// inside the line (the shown bytes, when the line was not cut), masks non-zero and without a
// bit at or above the query's positive-term count.  With tally: tally_off monotone from 0 to
// the keys' number, at most min(K, tally_words) words per query, every count >= 1, counts
// non-increasing with equal counts on ascending keys, their sum <= tally_tokens, tally_words <=
// tally_tokens, and tally_words == 0 exactly when tally_tokens == 0.
void validate_search(const SearchResult& r);
// The result lines of a search, one per query:
//   "print query: <terms joined by one space> \t hits: <h> \t lines: <l0> <l1> ...\n"
// (an `expr` query: its expression, SearchQuery::expr, in place of the joined terms)
// (a prefix term as it was asked: with its star; a pattern term as it was asked, too; a fuzzy
// term with its `~d`, a regex term between its slashes;
// <terms> are the positive terms, and a query
// with exclusion terms prints " \t not: <those joined by one space>" before " \t hits:")
// ranked (hits: the matches; nothing after "top:" when nothing matched):
//   "print query: <terms> \t hits: <matches> \t top: <l0>:<s0> <l1>:<s1> ...\n"
// A result with show prints one line per entry under its query's line:
//   "  <global line number>: <the shown bytes>\n"
// mark: the part of every span that lies inside the shown bytes stands between ">>" and "<<".
// A result with tally prints, under the query's line and its shown lines:
//   "  words: <tally_words> \t tokens: <tally_tokens>\n"
//   "  word: <key> \t count: <count>\n"   (one per returned word)
void format_search_output(const SearchResult& r, std::string* out, bool mark = false);

// Text read piece by piece (a file too large to hold): whole lines go straight into the
// engine's pinned staging, so host memory stays bounded by two chunks whatever the input.
class TextSource {
 public:
  virtual ~TextSource() = default;
  virtual u64 size() const = 0;  // total bytes (sizes the chunk bookkeeping)
  // Fills dst (room for cap bytes) with the next whole lines (the last line of the input
  // may lack its '\n'); returns the bytes written, 0 at the end.
  virtual u64 next(char* dst, u64 cap) = 0;
  virtual u64 lines() const = 0;  // lines handed out so far
};
// A file read with `threads` concurrent preads per chunk (0: up to 8); see io.cpp.
std::unique_ptr<TextSource> open_file_source(const std::string& path, u32 threads = 0);
// The same over the byte range [begin, end) of the file (begin at a line start).
std::unique_ptr<TextSource> open_file_range_source(const std::string& path, u64 begin, u64 end,
                                                   u32 threads = 0);

// ---- HBM budget planning (SURVEY.md §5.7 "HBM budget accounting per GPU") ----
// The reference sizes everything by compile-time constants (main.cu:18-20: 5,800 lines,
// 116,000 emits; three cudaMallocs at :393,402,451).  Here an engine's device pass is
// planned from its input size and the GPU's free memory before anything is allocated:
//  * the token buffers hold one map launch's worst case (a byte in two a token); a
//    streaming engine maps each chunk in windows of <= kStreamMapWindow bytes, so its
//    token buffers do not grow with --chunk-mb;
//  * the sort / reduce buffers of a dictionary engine hold the distinct keys only (ucap);
//    the reference algorithm's every-token buffers are made on first use
//    (DevicePipeline::ensure_radix_full);
//  * a one-pass input whose engine would not fit its share of HBM (free / hbm_share, at
//    most kHbmUsable of it), or that exceeds 2^30 tokens, is planned as a stream of
//    chunk_bytes chunks (default kDefaultStreamChunk) on the dictionary path; a plan that
//    still does not fit is refused with the sizes in the message.
struct DevicePassPlan {
  bool streaming = false;
  u64 chunk_bytes = 0;   // device text buffer: the one pass, or one stream chunk
  u64 pass_bytes = 0;    // largest input one pass takes (a streaming engine: map_window)
  u64 map_window = 0;    // a streamed chunk's map windows (0: not streaming)
  u64 cap_lines = 0;
  u64 cap = 0;           // tokens one map launch may emit
  u64 ucap = 0;          // distinct keys of the dictionary
  u64 rcap = 0;          // records the sort / reduce buffers hold
  u64 device_bytes = 0;  // the engine's planned device allocations
  u64 budget_bytes = 0;  // the HBM it may use
  std::string why;       // why the input was planned as a stream ("" if asked for)
};
constexpr u64 kStreamMapWindow = 32ull << 20;
constexpr u64 kDefaultStreamChunk = 256ull << 20;
constexpr double kHbmUsable = 0.9;
// free_bytes: the device's free memory (hipMemGetInfo).  Throws when no plan fits.
DevicePassPlan plan_device_pass(const JobConfig& cfg, u64 max_bytes, u64 max_lines,
                                u64 cap_records, u64 free_bytes);

class GpuWordCount {
 public:
  // Capacity is fixed at construction: max_text_bytes / max_lines per device pass.  With
  // the dictionary path and the fast map, larger inputs stream through in line-aligned
  // chunks of max_text_bytes (double-buffered H2D; one dictionary across chunks).
  GpuWordCount(const JobConfig& cfg, u64 max_text_bytes, u64 max_lines);
  ~GpuWordCount();
  GpuWordCount(const GpuWordCount&) = delete;
  GpuWordCount& operator=(const GpuWordCount&) = delete;

  WordCountResult run(const TextInput& in);
  // A streamed input (a streaming engine: JobConfig.chunk_bytes set, max_text_bytes larger
  // than it): chunks of chunk_bytes read from `src` into pinned staging, overlapped with
  // the H2D and the map of the previous chunk.
  WordCountResult run_source(TextSource& src);

  // How the engine's partition map has fared (diagnostics, tests): retunes of the map from
  // a job's output, jobs whose ordered build overflowed an LDS table and fell back to the
  // HBM table, and whether the in-job plan of large passes was given up.
  struct Stats {
    u32 retunes = 0, fallbacks = 0, planned_passes = 0;
    bool devplan_failed = false;
    // HBM: this engine's device allocations, and the GPU's free / total memory before them
    u64 device_bytes = 0, hbm_free = 0, hbm_total = 0;
    bool streaming = false;
    u64 chunk_bytes = 0, map_window = 0;
    // device bytes of the search stage's workspace (0 until the first search job)
    u64 search_bytes = 0;
    // device bytes of the index store (0 until the first append_index)
    u64 index_store_bytes = 0;
    // what the last Process stage of the reference algorithm (every token sorted) used:
    // "psort" (the partitioned LDS sort), "radix-host-plan" (the device-wide sort, live
    // passes launched from the plan read back) or "radix-device-plan" (every pass launched,
    // liveness and buffers decided on the device); "none" before the first such stage
    // (a dictionary job sorts no tokens)
    const char* process_path = "none";
  };
  Stats stats() const;

  // The partition map (kDictParts + 1 ascending range starts, partmap.hpp) -- a
  // load-balancing hint only: any ascending map gives the same results.  partition_map()
  // finishes a background retune first and returns false while the map is still the data-
  // independent default; set_partition_map() starts this engine on a map tuned earlier (the
  // CLI's per-file cache), returning false (map unchanged) for a malformed one.
  bool partition_map(std::vector<u64>* lo);
  bool set_partition_map(const std::vector<u64>& lo);

  // Stage split: map + process only, returning the sorted tokens of
  // this input; and reduce-only over (possibly unsorted) tokens.
  std::vector<PackedKey> run_map_stage(const TextInput& in, WordCountResult* stats);
  WordCountResult run_reduce_stage(const PackedKey* keys, u64 n);

  // Sort arbitrary packed keys on the device (used by tests and the shuffle receiver).
  // counts (n of them, optional) travel with their keys: *sorted_counts gets them in
  // sorted order, through the sort's fused count gather.
  std::vector<u32> sort_keys(const PackedKey* keys, u64 n, std::vector<PackedKey>* sorted,
                             const u64* counts = nullptr,
                             std::vector<u64>* sorted_counts = nullptr);

  // Single-stage entry points for the kernel unit tests.
  // Stable compaction of the compat map's fixed slots (main.cu:411): slot_keys holds
  // num_lines * emits_per_line keys, the first line_counts[l] slots of line l are live.
  // Needs a MapPath::kCompat engine with capacity for num_lines lines.
  std::vector<PackedKey> compact_slots(const u32* line_counts, u32 num_lines,
                                       const PackedKey* slot_keys);
  // Reduce steps over keys that are already sorted: boundary mark + head compaction +
  // adjacent difference (main.cu:161-238, 462) on the configured reduce path.
  WordCountResult reduce_sorted(const PackedKey* sorted, u64 n);
  // Root merge of the gather strategy (launch_merge_sorted_runs) over host-made runs, each
  // sorted with distinct keys: the merged (key, val, count) entries.
  WordCountResult merge_runs(const std::vector<std::vector<KeyCount>>& runs);
  // The device selection alone (kernels/topk.hip) over host-made records sorted by key
  // with distinct keys: their top k (k <= kTopKMax, n within the engine's capacity).
  TopResult top_counts(const KeyCount* recs, u64 n, u32 k);

  // A whole job whose full records never cross PCIe: the key-ordered records stay in
  // device memory, the selection kernels pick the top k (1 <= k <= kTopKMax) there and
  // only those travel.  Dictionary engines (sort=dict, either map path); inputs past one
  // pass and sources stream like run() / run_source().
  TopResult run_top(const TextInput& in, u32 k);
  TopResult run_top_source(TextSource& src, u32 k);

  // The word job, then the inverted index of the same text on the device (kernels/
  // index.hip): the records stay in device memory, the text is tokenised once more with
  // each token's line, and the (word rank, line) pairs are sorted there.  Dictionary
  // engines with the fast map, word keys (ngram 1), one pass (in.bytes within the engine's
  // pass; larger inputs and sources: the CPU engine).
  IndexResult run_index(const TextInput& in);

  // run_index's word job and index stage, then the search stage over the index in device
  // memory (kernels/search.hip): up to kSearchMaxQueries queries; only the answers, the
  // per-term counts and the counters cross PCIe.  run_index's refusals apply.  The text
  // stays in device memory beside the index (the engine's own copy, not the staging
  // buffer): phrase queries are verified against it.
  // show = N: the show stage behind it ("show": kernels/show.hip).
  // tally = K: the tally stage behind both ("tally": kernels/tally.hip).
  SearchResult run_search(const TextInput& in, const std::vector<SearchQuery>& queries,
                          u64 rank_k = 0, bool ignore_case = false, u64 show = 0,
                          u64 tally = 0, u32 by_file = 0);
  // Another batch from the index this engine's last job left on the device.  That job must
  // have been a run_index or a run_search: any other job (a refused one that had started
  // to write included) marks the index stale, and this then throws.
  SearchResult search_resident(const std::vector<SearchQuery>& queries, u64 rank_k = 0,
                               bool ignore_case = false, u64 show = 0, u64 tally = 0,
                               u32 by_file = 0);
  // One more block of whole lines into the resident index ("appending to the index" above):
  // the block's word job and index stage, then the merge on the device into the engine's
  // index store.  in.first_line must be the resident first_line + lines.
  // new_file: the block begins a segment ("corpus"); else it extends the last one.
  IndexAppend append_index(const TextInput& in, bool new_file = false);
  // The resident index's segment table ("corpus"); throws when the index is stale.
  IndexSegments segments() const;
  // The oldest `lines` lines out of the resident index ("dropping the oldest lines" above):
  // compacted on the device into the other half of the engine's index store.
  IndexDrop drop_index(u64 lines);
  // The resident index downloaded (entries, postings, statistics), whatever it was built from;
  // throws as search_resident does when it is stale.
  IndexResult index_resident();

  const JobConfig& config() const;
  u64 token_capacity() const;
  u64 text_capacity() const;  // bytes per device pass (input_buffer() size)
  // Pinned host staging buffer of the text (capacity max_text_bytes + 64).  A TextInput
  // whose data points here is uploaded without the host-side staging copy -- the
  // analogue of the reference loading the file into its host array before any timer.
  char* input_buffer();

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

// Input text in page-locked host memory: the GPU engine DMAs it (whole, or chunk by chunk
// when streaming) without a staging copy.  Falls back to ordinary memory when no GPU
// runtime is present (CPU engine, build machine).
class HostText {
 public:
  explicit HostText(u64 capacity);
  ~HostText();
  HostText(const HostText&) = delete;
  HostText& operator=(const HostText&) = delete;
  char* data() { return data_; }
  const char* data() const { return data_; }
  u64 size() const { return size_; }
  u64 lines() const { return lines_; }
  u64 capacity() const { return cap_; }
  bool pinned() const { return pinned_; }
  void set_size(u64 bytes, u64 lines);
  TextInput input(u64 first_line = 0) const;

 private:
  char* data_ = nullptr;
  u64 cap_ = 0, size_ = 0, lines_ = 0;
  bool pinned_ = false;
};

class CpuWordCount {
 public:
  explicit CpuWordCount(const JobConfig& cfg);
  WordCountResult run(const TextInput& in);
  TopResult run_top(const TextInput& in, u64 k);  // run() + the host selection, any k
  // The inverted index on the host, any size: (key, line) pairs, one stable sort by key.
  // Word keys only (ngram == 1), like the GPU job.
  IndexResult run_index(const TextInput& in);
  // run_index() + the host evaluation (search_index with the text), any size, any number
  // of queries and every mode.
  SearchResult run_search(const TextInput& in, const std::vector<SearchQuery>& queries,
                          u64 rank_k = 0, bool ignore_case = false, u64 show = 0,
                          u64 tally = 0, u32 by_file = 0);
  std::vector<PackedKey> run_map_stage(const TextInput& in, WordCountResult* stats);
  WordCountResult run_reduce_stage(const PackedKey* keys, u64 n);

 private:
  JobConfig cfg_;
};

// Tokenize one line with the reference rules (delimiters, emit cap, truncation).  Used by
// the CPU engine and the tests; returns the number of tokens dropped by the emit cap.
// at (word keys only): per emitted token its byte offset in the line and its full length.
int tokenize_line(const char* line, u64 len, const JobConfig& cfg, std::vector<PackedKey>* out,
                  u64* truncated, std::vector<std::pair<u32, u32>>* at = nullptr);

// Sorted unique keys + counts -> entries with val = exclusive prefix of counts.
void entries_from_sorted_tokens(const PackedKey* sorted, u64 n, std::vector<WordCountEntry>* out);

// Device self-test of the string library: one GPU thread per
// string runs d_strlen / d_strcmp (with the next string) / d_strcpy_bounded / d_strtok_r /
// d_itoa; the rows come back for comparison with the host build.
constexpr int kStringTestMax = 128;
struct StringTestOut {
  int len, cmp_next, copy_len, ntok;
  int tok_off[8];
  char copy[30];
  char itoa_buf[34];
};
std::vector<StringTestOut> run_string_selftest(const std::vector<std::string>& strings,
                                               const std::vector<int>& ints,
                                               const std::string& delims, int device = 0);

}  // namespace locust
