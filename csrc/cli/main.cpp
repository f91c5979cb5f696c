// ./MapReduce -- command line driver (SURVEY.md §2.6 API surface; /root/reference/
// MapReduce/src/main.cu:358-532).
//
// Positional CLI of the reference, byte-compatible stdout:
//   MapReduce <file>                                   whole file, one process
//   MapReduce <file> <line_start> <line_end>           window [start, end)
//   MapReduce <file> <start> <end> <node_num> <stage>  stage 0 = all, 1 = map only
//                                                      (writes a spill), 2 = reduce only
// plus long flags (runtime switches replacing the reference's #defines):
//   --backend gpu|cpu  --reduce-path lds|global  --map-path compat|fast
//   --sort radix|dict  --gpus N  --comm auto|rccl|loopback  --strategy auto|gather|shuffle
//   --emits-per-line N  --max-key N  --ref-compat
//   --stage map|reduce  --spill-dir DIR  --spill-format text|binary|kiv  --inputs a,b,...
//   --export-kiv FILE (results as the reference's 40-B KeyIntValuePair records)
//   --warmup N  --iters N  --json FILE  --quiet  --check  --device N  --chunk-mb N
//   --ref-timers (stage times taken where the reference's host timers were)
//   --top K (the K most frequent words instead of the whole dictionary, rank order)
//   --ngram N (count the word N-grams of each line, N <= 3, instead of its words)
//   --index (the inverted index: every word with the lines it occurs on)
//   --search "w1 w2" [--match all|any|phrase|near] (the lines that hold all / any of the
//     words, the words as consecutive tokens in that order, or the words within --within W
//     tokens of one another; repeat --search for a batch: answered from the index on the
//     device, or by --backend cpu)
//     --match expr: the argument is a Boolean expression, "( to AND be ) OR ( Ham* AND NOT Hamlet )"
//   --within W (with --match near: the window in tokens, W >= 1)
//   --not "w1 w2" (after a --search: lines that hold one of these words are no answer of it)
//   --rank K (with --search: each query's K best lines with their scores, best first)
//   --wildcard (with --search: a word that ends in * is a prefix term, "ham*")
//   --glob (with --search: * and ? anywhere in a word, "*ing", "h?mlet"; a superset of --wildcard)
//   --fuzzy (with --search: a word that ends in ~1 or ~2 also finds the words within that many
//            byte edits of it, "Hamlet~1", "quene~2")
//   --regex (with --search: a word written /re/ is a regular expression over whole words,
//            "/(king|queen)[!?]?/", "/[A-Z][A-Z]+/")
//   --ignore-case (with --search: the ASCII letters of every word match either case)
//   --show N (with --search: under each query's line, every returned line's first N bytes)
//   --mark (with --show: the matching tokens of a shown line stand between >> and <<)
//   --tally K (with --search: under each query's line, the K most frequent words of its lines)
//   --block-kb N (with --index or --search: the index is built from line-aligned blocks of at
//     most N KiB, the first indexed, the rest appended to the index in device memory)
//   --keep-blocks M (with --block-kb: a sliding window -- once more than M blocks are resident the
//     oldest block's lines are dropped from the index, on the device)
// and a synthetic-text generator (BASELINE configs "1M lines" / "10 GB"):
//   MapReduce --gen FILE (--gen-lines N | --gen-bytes N) [--seed S] [--vocab V]
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "locust/dist.hpp"
#include "locust/engine.hpp"
#include "locust/gen.hpp"
#include "locust/io.hpp"
#include "locust/stage.hpp"

using namespace locust;

namespace {

unsigned long long peak_rss_kb();

// A one-shot GPU run ends with _exit once its output is flushed (the
// HIP runtime's teardown -- streams, pinned and device memory, code objects -- took most of
// the ~80 ms outside main()).  Off with LOCUST_FAST_EXIT=0, and under a profiler (rocprofv3
// preloads its tool library and flushes its traces at the runtime's exit).
bool fast_exit_ok() {
  if (const char* e = std::getenv("LOCUST_FAST_EXIT"))
    if (e[0] == '0') return false;
  if (const char* p = std::getenv("LD_PRELOAD"))
    if (std::strstr(p, "rocprof") || std::strstr(p, "roctracer")) return false;
  for (char** e = environ; e && *e; ++e)
    if (std::strncmp(*e, "ROCPROF", 7) == 0) return false;
  return true;
}
bool g_fast_exit = false;  // run() left its GPU state for the process exit to reclaim

struct CliArgs {
  std::string file;
  i64 line_start = -1, line_end = -1;
  int node = 0;
  int stage = 0;
  bool window = false;
  bool byte_range = false;  // --byte-range A:B (stage 1): a byte window instead of lines
  u64 byte_begin = 0, byte_end = ~0ull;
  JobConfig cfg;
  int gpus = 1;
  bool gpus_given = false;   // --gpus on the command line (even --gpus 1: RCCL rank)
  LocalComm comm = LocalComm::kAuto;
  DistStrategy strategy = DistStrategy::kAuto;  // --gpus N: after-map strategy (--strategy)
  std::string spill_dir = "/tmp";
  SpillFormat spill_fmt = SpillFormat::kText;
  std::vector<std::string> inputs;
  int reducer = 0, reducers = 1;  // --reducer r/R: key range r of R (stage 2)
  std::string result_file;        // --result-file: the result lines go there, not stdout
  int out_format = 0;             // --output-format: 0 by mode, 1 gpu (with val), 2 cpu
  int warmup = 0, iters = 1;
  std::string json;
  std::string export_kiv;  // final results as KeyIntValuePair records (--export-kiv FILE)
  bool quiet = false;
  u64 top = 0;  // --top K: the result lines are the K most frequent words (0: all)
  bool index = false;  // --index: the result lines carry every word's line numbers
  // --search "w1 w2" (repeatable): the result lines are the queries' answers
  std::vector<std::string> search_args;
  // corpus: --add FILE (repeatable) names the files behind the first; --in "PATH ..." belongs to
  // the --search before it; --by-file / --count ask for answers by file
  std::vector<std::string> add;
  std::vector<std::string> in_args;
  u32 by_file = 0;  // kByFileNone / kByFile / kByFileCount
  std::vector<std::string> not_args;  // parallel: the --not words of each --search, joined by ' '
  std::vector<SearchQuery> queries;
  std::string match;  // --match all|any|phrase|near ("": all)
  bool within_given = false;
  u64 within = 0;  // --within W: the window of --match near, in tokens
  bool rank_given = false;
  u64 rank = 0;  // --rank K: every query answers its K best lines, scored (0: all its lines)
  bool wildcard = false;  // --wildcard: a --search word that ends in * is a prefix term
  bool glob = false;      // --glob: * and ? anywhere in a --search word (pattern terms)
  bool fuzzy = false;     // --fuzzy: a --search word that ends in ~1 or ~2 is a fuzzy term
  bool regex = false;     // --regex: a --search word written /re/ is a regex term
  bool ignore_case = false;  // --ignore-case: the batch's ASCII letters match either case
  u64 show = 0;       // --show N: the returned lines' first N bytes (0: line numbers only)
  bool mark = false;  // --mark: the shown lines' matching tokens between >> and <<
  u64 tally = 0;      // --tally K: the K most frequent words of every query's returned lines
  bool block_given = false;
  u64 block_kb = 0;   // --block-kb N: --index / --search build the index in blocks of N KiB
  bool keep_given = false;
  u64 keep_blocks = 0;  // --keep-blocks M: at most M blocks stay in the index (0: all of them)
  std::string gen_out;  // generator mode
  GenSpec gen;
};

void usage() {
  std::printf("Missing or invalid arguments.\n");
  std::printf("mapreduce <filename> [line_start] [line_end] [node_num] [stage]\n");
}

void help() {
  std::printf(
      "usage: MapReduce <file> [line_start line_end [node_num stage]] [flags]\n"
      "       MapReduce --gen FILE (--gen-lines N | --gen-bytes N) [--seed S] [--vocab V]\n"
      "\n"
      "  stage 0: the whole job; 1: map only, writes the combined spill <spill-dir>/out.<node>.*\n"
      "  and its index; 2: reduce only, merges spills (--inputs a,b,... or out.<node>.*)\n"
      "\n"
      "  --backend gpu|cpu          --reduce-path lds|global   --map-path fast|compat\n"
      "  --sort dict|radix          --gpus N                   --comm auto|loopback|rccl\n"
      "  --strategy auto|gather|shuffle                        --device N\n"
      "  --emits-per-line N         --max-key N                --ref-compat\n"
      "  --stage map|reduce         --spill-dir DIR            --spill-format text|binary|kiv\n"
      "  --inputs a,b,...           --reducer r/R              --result-file FILE\n"
      "  --byte-range A:B           (stage 1: bytes [A, B) moved to line starts; B empty: EOF)\n"
      "  --output-format gpu|cpu    (result lines with val, or the CPU build's)\n"
      "  --export-kiv FILE          --json FILE|-              --quiet --check --combine\n"
      "  --warmup N --iters N       --chunk-mb N               --ref-timers\n"
      "  --top K                    (only the K most frequent words, count descending, ties\n"
      "                             by key; selected on the device on one GPU, K <= %u)\n"
      "  --ngram N                  (count word N-grams, N in [1, %d]: N consecutive words of one\n"
      "                             line joined by single spaces; never across a line end.  A\n"
      "                             key is the first --max-key bytes of the joined words.  Not\n"
      "                             with --map-path compat or the stage split)\n"
      "  --index                    (inverted index: after each word its count and the 0-based\n"
      "                             numbers of the lines it occurs on, one per occurrence; whole\n"
      "                             one-pass jobs on one GPU or --backend cpu.  Not with --top,\n"
      "                             --ngram N > 1, the stage split, --gpus N > 1, --chunk-mb,\n"
      "                             --sort radix or --map-path compat)\n"
      "  --search \"w1 w2 ...\"       (the 0-based lines that hold the words, 1 to 8 of them, split\n"
      "                             like the text; repeat --search for a batch.  Answered from the\n"
      "                             index in device memory, or by --backend cpu.  Restrictions\n"
      "                             as --index, and not with --index)\n"
      "  --match all|any|phrase|near|expr\n"
      "                             (--search: lines with every word (default), with any, with\n"
      "                             the words as consecutive tokens in the order given, whatever\n"
      "                             delimiters stand between them, or with every word inside some\n"
      "                             --within W consecutive tokens of the line, in any order.\n"
      "                             expr: the --search argument is a Boolean expression over up to\n"
      "                             8 words, \"( to AND be ) OR ( Ham* AND NOT Hamlet )\": AND, OR\n"
      "                             and NOT in upper case, NOT > AND > OR, parentheses, words side\n"
      "                             by side joined by AND; split at blanks and parentheses only.\n"
      "                             Refused: an expression true of a line with none of its words\n"
      "                             (\"NOT a\"), and --not or --within with it.  With --rank,\n"
      "                             --show, --wildcard, --glob, --fuzzy, --ignore-case)\n"
      "  --within W                 (--match near, which needs it: the window in tokens,\n"
      "                             1 <= W < 2^32; with W = 2 two words must be neighbours)\n"
      "  --not \"w1 w2 ...\"          (exclusion words of the nearest --search before it, split\n"
      "                             like the text: a line that holds one of them is no answer of\n"
      "                             that query, whatever --match says.  Repeatable: the words add\n"
      "                             up; a query takes 8 words in all.  A word found nowhere takes\n"
      "                             nothing away.  With every --match, --within, --rank, --wildcard\n"
      "                             and --backend cpu; taken away on the device before a phrase is\n"
      "                             verified or a line is scored)\n"
      "  --rank K                   (--search: only each query's K best lines, best first, as\n"
      "                             line:score; a line's score adds, per distinct word of the\n"
      "                             query, its occurrences on the line times a weight that grows\n"
      "                             with the word's rarity.  Scored and selected on the device on\n"
      "                             one GPU, or by --backend cpu; K >= 1)\n"
      "  --wildcard                 (--search: a word that ends in * stands for every word that\n"
      "                             starts with what precedes the star, \"ham*\": it counts as\n"
      "                             one word whose lines are all of theirs.  A lone * is refused,\n"
      "                             a * anywhere else is literal.  With every --match and --rank)\n"
      "  --glob                     (--search: * stands for any run of bytes, the empty one too,\n"
      "                             and ? for exactly one byte, anywhere in a word: \"*ing\",\n"
      "                             \"h?mlet\", \"*aml*\".  Such a word counts as one word whose\n"
      "                             lines are those of every word the whole pattern matches; the\n"
      "                             device scans the dictionary for them.  \"ham*\" stays the\n"
      "                             prefix word of --wildcard, which --glob includes.  A pattern\n"
      "                             is never cut: one longer than the key length is refused, and so\n"
      "                             is one of stars alone.  With every --match, --rank, --not,\n"
      "                             --within and --backend cpu; --rank then takes\n"
      "                             --emits-per-line <= 8192)\n"
      "  --fuzzy                    (--search: a word that ends in ~1 or ~2 stands for every word\n"
      "                             within that many edits of what precedes the ~ -- one byte\n"
      "                             inserted, deleted or replaced is one edit: \"Hamlet~1\" finds\n"
      "                             Hamlet! and [Hamlet too, \"quene~2\" finds queen.  It counts as\n"
      "                             one word whose lines are all of theirs; the device scans the\n"
      "                             dictionary for them.  The word is never cut and is longer than\n"
      "                             its budget; another digit than 1 or 2 is refused, and so is a *\n"
      "                             or ? in the word under --wildcard or --glob.  A ~ anywhere else\n"
      "                             is literal.  With everything --glob goes with, and --glob)\n"
      "  --regex                    (--search: a word written /re/ is a regular expression that a\n"
      "                             whole word must match: literals, \\x escapes, ., [a-z], [^...],\n"
      "                             ( ), |, *, + and ?, over bytes, at most 32 positions and 128\n"
      "                             bytes: \"/(king|queen)[!?]?/\", \"/[A-Z][A-Z]+/\".  Delimiters and\n"
      "                             blanks between the slashes belong to it; write \\/ for a slash.\n"
      "                             It counts as one word whose lines are all of its words'; the\n"
      "                             device scans the dictionary for them.  {m,n}, anchors, \\d and\n"
      "                             \\w are refused.  With everything --glob goes with, --glob and\n"
      "                             --fuzzy)\n"
      "  --show N                   (--search: under each query's result line, one line per\n"
      "                             returned line: two spaces, its number, \": \" and its first N\n"
      "                             bytes, 1 <= N <= 65536; the lines are gathered on the device.\n"
      "                             With every --match, --rank (the winners, in rank order),\n"
      "                             --not, --wildcard, --glob, --fuzzy and --ignore-case)\n"
      "  --mark                     (--show: every token of a shown line that matches one of the\n"
      "                             query's words -- not its --not words -- stands between >>\n"
      "                             and <<, as far as it lies inside the N bytes)\n"
      "  --tally K                  (--search: under each query's result line and its shown\n"
      "                             lines, \"  words: W \\t tokens: T\" -- the distinct words and\n"
      "                             the tokens of the lines the query returns -- and the K most\n"
      "                             frequent of those words, \"  word: <key> \\t count: <n>\", by\n"
      "                             count and then by key, 1 <= K <= 4096; counted on the device.\n"
      "                             With every --match, --rank (the winners' words), --show,\n"
      "                             --not and both backends)\n"
      "  --block-kb N               (--index, --search: the index is built block by block -- the\n"
      "                             text is cut into blocks of whole lines of at most N KiB, N >= 1,\n"
      "                             the first is indexed and every further one indexed alone and\n"
      "                             merged into the index in device memory, so the engine is sized to\n"
      "                             one block and the text need not fit one device pass, only device\n"
      "                             memory.  The result lines are those of the run without it.  A line\n"
      "                             longer than a block is refused.  With --backend cpu the blocks'\n"
      "                             indexes are merged on the host.  Not with --chunk-mb)\n"
      "  --add FILE                 (--index / --search, repeatable: one more file behind the first\n"
      "                             in the same index; lines are numbered through the corpus, every\n"
      "                             file is cut into blocks of its own with --block-kb; not with a\n"
      "                             line window, --chunk-mb, --gpus N, the stage split or --top)\n"
      "  --in \"PATH ...\"            (the --search before it is answered from these files only,\n"
      "                             named as on the command line)\n"
      "  --by-file                  (--search: under each query's line one line per file with a hit:\n"
      "                             its hits and their numbers inside the file; --show prints\n"
      "                             <path>:<local>: in front of a shown line)\n"
      "  --count                    (--by-file, and only the counts: hits per query and per file)\n"
      "  --keep-blocks M            (--block-kb: a sliding window over the text -- whenever an append\n"
      "                             leaves more than M blocks in the index, M >= 1, the oldest block's\n"
      "                             lines are dropped from it: their postings, the words that empty\n"
      "                             out, their text and line starts, compacted on the device.  The\n"
      "                             result lines are those of the run without --block-kb and\n"
      "                             --keep-blocks over the lines from the first line of block\n"
      "                             blocks - M on; line numbers stay global.  With --backend cpu the\n"
      "                             merged index is trimmed on the host)\n"
      "  --ignore-case              (--search: the ASCII letters of every word of every query,\n"
      "                             --not words too, match either case: \"to be\" finds \"To be\".\n"
      "                             Other bytes match only themselves.  With --glob, --wildcard and\n"
      "                             everything --glob goes with)\n"
      "  --help\n"
      "\n"
      "Environment: LOCUST_LOG=info|debug and the LOCUST_* switches in docs/ENVIRONMENT.md.\n",
      (unsigned)kTopKMax, kMaxNgram);
}

std::vector<std::string> split(const std::string& s, char c) {
  std::vector<std::string> out;
  size_t p = 0;
  while (p <= s.size()) {
    size_t q = s.find(c, p);
    if (q == std::string::npos) q = s.size();
    if (q > p) out.push_back(s.substr(p, q - p));
    p = q + 1;
  }
  return out;
}

bool parse(int argc, char** argv, CliArgs* a) {
  std::vector<std::string> pos;
  apply_env_overrides(a->cfg);
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    auto need = [&](const char* name) -> std::string {
      if (i + 1 >= argc) throw Error(std::string("missing value for ") + name);
      return argv[++i];
    };
    if (s == "--backend") {
      std::string v = need("--backend");
      a->cfg.backend = v == "cpu" ? Backend::kCpu : Backend::kGpu;
    } else if (s == "--reduce-path") {
      a->cfg.reduce_path = need("--reduce-path") == "global" ? ReducePath::kGlobal : ReducePath::kLds;
    } else if (s == "--map-path") {
      a->cfg.map_path = need("--map-path") == "compat" ? MapPath::kCompat : MapPath::kFast;
    } else if (s == "--sort") {
      a->cfg.sort_path = need("--sort") == "dict" ? SortPath::kDict : SortPath::kRadix;
    } else if (s == "--gpus") {
      a->gpus = std::atoi(need("--gpus").c_str());
      a->gpus_given = true;
    } else if (s == "--comm") {
      const std::string v = need("--comm");
      a->comm = v == "rccl" ? LocalComm::kRccl : v == "loopback" ? LocalComm::kLoopback
                                                               : LocalComm::kAuto;
    } else if (s == "--strategy") {
      const std::string v = need("--strategy");
      if (v != "auto" && v != "gather" && v != "shuffle") throw Error("--strategy auto|gather|shuffle");
      a->strategy = v == "gather" ? DistStrategy::kGather : v == "shuffle" ? DistStrategy::kShuffle
                                                                          : DistStrategy::kAuto;
    } else if (s == "--device") {
      a->cfg.device = std::atoi(need("--device").c_str());
    } else if (s == "--emits-per-line") {
      a->cfg.emits_per_line = std::atoi(need("--emits-per-line").c_str());
    } else if (s == "--max-key") {
      a->cfg.max_key_len = std::atoi(need("--max-key").c_str());
    } else if (s == "--ref-compat") {
      a->cfg.ref_compat = true;
    } else if (s == "--check") {
      a->cfg.check = true;
    } else if (s == "--combine") {
      a->cfg.combine = true;
    } else if (s == "--no-sync-plan") {
      a->cfg.sync_plan = false;
    } else if (s == "--stage") {
      std::string v = need("--stage");
      a->stage = v == "map" || v == "1" ? 1 : (v == "reduce" || v == "2" ? 2 : 0);
    } else if (s == "--spill-dir") {
      a->spill_dir = need("--spill-dir");
    } else if (s == "--spill-format") {
      const std::string v = need("--spill-format");
      a->spill_fmt = v == "binary" ? SpillFormat::kBinary : v == "kiv" ? SpillFormat::kKiv
                                                                     : SpillFormat::kText;
    } else if (s == "--export-kiv") {
      a->export_kiv = need("--export-kiv");
    } else if (s == "--inputs") {
      a->inputs = split(need("--inputs"), ',');
    } else if (s == "--reducer") {
      const std::string v = need("--reducer");
      const size_t sl = v.find('/');
      if (sl == std::string::npos) throw Error("--reducer r/R");
      a->reducer = std::atoi(v.substr(0, sl).c_str());
      a->reducers = std::atoi(v.substr(sl + 1).c_str());
      if (a->reducers < 1 || a->reducer < 0 || a->reducer >= a->reducers)
        throw Error("--reducer r/R needs 0 <= r < R");
    } else if (s == "--byte-range") {
      const std::string v = need("--byte-range");
      const size_t c = v.find(':');
      if (c == std::string::npos || c == 0) throw Error("--byte-range A:B");
      char* endp = nullptr;
      a->byte_begin = std::strtoull(v.c_str(), &endp, 10);
      if (endp != v.c_str() + c) throw Error("--byte-range A:B");
      if (c + 1 < v.size()) {
        a->byte_end = std::strtoull(v.c_str() + c + 1, &endp, 10);
        if (*endp) throw Error("--byte-range A:B");
      }
      if (a->byte_end < a->byte_begin) throw Error("--byte-range A:B needs A <= B");
      a->byte_range = true;
    } else if (s == "--result-file") {
      a->result_file = need("--result-file");
    } else if (s == "--output-format") {
      const std::string v = need("--output-format");
      if (v != "gpu" && v != "cpu") throw Error("--output-format gpu|cpu");
      a->out_format = v == "gpu" ? 1 : 2;
    } else if (s == "--warmup") {
      a->warmup = std::atoi(need("--warmup").c_str());
    } else if (s == "--iters") {
      a->iters = std::max(1, std::atoi(need("--iters").c_str()));
    } else if (s == "--json") {
      a->json = need("--json");
    } else if (s == "--quiet") {
      a->quiet = true;
    } else if (s == "--ref-timers") {
      a->cfg.ref_timers = true;
    } else if (s == "--top") {
      const std::string v = need("--top");
      char* endp = nullptr;
      const long long k = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || k < 1) throw Error("--top K needs an integer K >= 1");
      a->top = (u64)k;
    } else if (s == "--index") {
      a->index = true;
    } else if (s == "--search") {
      a->search_args.push_back(need("--search"));
      a->not_args.emplace_back();
      a->in_args.emplace_back();
    } else if (s == "--add") {
      a->add.push_back(need("--add"));
    } else if (s == "--by-file") {
      a->by_file = std::max(a->by_file, kByFile);
    } else if (s == "--count") {
      a->by_file = kByFileCount;
    } else if (s == "--in") {
      const std::string v = need("--in");
      if (a->search_args.empty())
        throw Error("--in \"" + v + "\" names the files that the --search before it is "
                    "answered from: give --search first");
      a->in_args.back() += " " + v;
    } else if (s == "--not") {
      const std::string v = need("--not");
      if (a->search_args.empty())
        throw Error("--not \"" + v + "\" names words that the --search before it must not "
                    "find on a line: give --search first");
      a->not_args.back() += " " + v;
    } else if (s == "--match") {
      a->match = need("--match");
      if (a->match != "all" && a->match != "any" && a->match != "phrase" && a->match != "near" &&
          a->match != "expr")
        throw Error("--match takes all, any, phrase, near or expr (how --search combines its "
                    "words; expr: the --search argument is a Boolean expression)");
    } else if (s == "--within") {
      const std::string v = need("--within");
      char* endp = nullptr;
      const long long w = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || w < 1 || w > (long long)kSearchMaxWithin)
        throw Error("--within W (the window of --match near, in tokens) needs an integer W "
                    "with 1 <= W < 2^32");
      a->within = (u64)w;
      a->within_given = true;
    } else if (s == "--wildcard") {
      a->wildcard = true;
    } else if (s == "--glob") {
      a->glob = true;
    } else if (s == "--fuzzy") {
      a->fuzzy = true;
    } else if (s == "--regex") {
      a->regex = true;
    } else if (s == "--ignore-case") {
      a->ignore_case = true;
    } else if (s == "--show") {
      const std::string v = need("--show");
      char* endp = nullptr;
      const long long n = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || n < 1 || n > (long long)kShowMaxBytes)
        throw Error("--show N (the first N bytes of every line a --search query returns) needs "
                    "an integer N with 1 <= N <= " + std::to_string(kShowMaxBytes));
      a->show = (u64)n;
    } else if (s == "--tally") {
      const std::string v = need("--tally");
      char* endp = nullptr;
      const long long n = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || n < 1 || n > (long long)kTopKMax)
        throw Error("--tally K (the K most frequent words of the lines every --search query "
                    "returns) needs an integer K with 1 <= K <= " + std::to_string(kTopKMax));
      a->tally = (u64)n;
    } else if (s == "--mark") {
      a->mark = true;
    } else if (s == "--rank") {
      const std::string v = need("--rank");
      char* endp = nullptr;
      const long long k = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || k < 1 || k > 0xffffffffll)
        throw Error("--rank K (the best K lines of every --search query) needs an integer K "
                    "with 1 <= K < 2^32");
      a->rank = (u64)k;
      a->rank_given = true;
    } else if (s == "--ngram") {
      const std::string v = need("--ngram");
      char* endp = nullptr;
      const long long n = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || n < 1 || n > kMaxNgram)
        throw Error("--ngram N needs an integer N in [1, " + std::to_string(kMaxNgram) + "]");
      a->cfg.ngram = (int)n;
    } else if (s == "--chunk-mb") {
      a->cfg.chunk_bytes = (u64)std::atoll(need("--chunk-mb").c_str()) << 20;
    } else if (s == "--block-kb") {
      const std::string v = need("--block-kb");
      char* endp = nullptr;
      const long long n = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || n < 1 || n > (1ll << 40))
        throw Error("--block-kb N needs an integer N >= 1 (KiB per block)");
      a->block_given = true;
      a->block_kb = (u64)n;
    } else if (s == "--keep-blocks") {
      const std::string v = need("--keep-blocks");
      char* endp = nullptr;
      const long long n = std::strtoll(v.c_str(), &endp, 10);
      if (v.empty() || *endp || n < 1 || n > (1ll << 40))
        throw Error("--keep-blocks M needs an integer M >= 1 (blocks kept in the index)");
      a->keep_given = true;
      a->keep_blocks = (u64)n;
    } else if (s == "--gen") {
      a->gen_out = need("--gen");
    } else if (s == "--gen-lines") {
      a->gen.lines = (u64)std::atoll(need("--gen-lines").c_str());
    } else if (s == "--gen-bytes") {
      a->gen.bytes = (u64)std::atoll(need("--gen-bytes").c_str());
    } else if (s == "--seed") {
      a->gen.seed = (u64)std::atoll(need("--seed").c_str());
    } else if (s == "--vocab") {
      a->gen.vocab = (u32)std::atoll(need("--vocab").c_str());
    } else if (s.size() > 2 && s[0] == '-' && s[1] == '-') {
      throw Error("unknown flag " + s);
    } else {
      pos.push_back(s);
    }
  }
  if (a->cfg.emits_per_line <= 0) throw Error("--emits-per-line must be > 0");
  if (a->cfg.max_key_len < 1 || a->cfg.max_key_len > kKeyBytes - 1)
    throw Error("--max-key must be in [1, " + std::to_string(kKeyBytes - 1) + "]");
  if (!a->gen_out.empty()) return true;
  if (pos.empty()) return false;
  a->file = pos[0];
  if (pos.size() > 1) {
    a->window = true;
    a->line_start = std::strtol(pos[1].c_str(), nullptr, 10);
    a->line_end = pos.size() > 2 ? std::strtol(pos[2].c_str(), nullptr, 10) : -1;
  }
  if (pos.size() > 3) {
    a->node = (int)std::strtol(pos[3].c_str(), nullptr, 10);
    if (pos.size() > 4) a->stage = (int)std::strtol(pos[4].c_str(), nullptr, 10);
  }
  if (a->top) {
    if (a->stage == 1) throw Error("--top selects from a result: not with stage 1 (map only)");
    if (!a->export_kiv.empty()) throw Error("--top and --export-kiv do not combine");
    if (a->cfg.ref_timers) throw Error("--top and --ref-timers do not combine");
    if (a->cfg.backend == Backend::kGpu && a->cfg.sort_path == SortPath::kRadix)
      throw Error("--top on the GPU needs the dictionary path (--sort dict)");
  }
  if (a->cfg.ngram > 1) {
    // the text spill cannot carry keys with spaces, so the stage split stays a word job
    if (a->stage != 0 || !a->inputs.empty() || a->reducers > 1)
      throw Error("--ngram N > 1 runs whole jobs only: not with the stage split (stage 1 or 2, "
                  "--stage, --inputs, --reducer)");
    if (a->cfg.backend == Backend::kGpu && a->cfg.map_path == MapPath::kCompat)
      throw Error("--ngram N > 1 needs the fast map (map_path fast), not --map-path compat");
  }
  if (!a->match.empty() && a->search_args.empty())
    throw Error("--match selects how --search combines its words: give --search too");
  if (a->within_given && a->match != "near")
    throw Error("--within W is the window of --match near: give --match near too");
  if (a->match == "near" && !a->within_given)
    throw Error("--match near needs its window: give --within W too (W tokens, W >= 1)");
  if (a->rank_given && a->search_args.empty())
    throw Error("--rank K selects the best lines of a --search query: give --search too");
  if (a->wildcard && a->search_args.empty())
    throw Error("--wildcard selects how --search reads a word that ends in *: give --search too");
  if (a->glob && a->search_args.empty())
    throw Error("--glob selects how --search reads * and ? in a word: give --search too");
  if (a->fuzzy && a->search_args.empty())
    throw Error("--fuzzy selects how --search reads a word that ends in ~1 or ~2: give --search too");
  if (a->regex && a->search_args.empty())
    throw Error("--regex selects how --search reads a word written /re/: give --search too");
  if (a->ignore_case && a->search_args.empty())
    throw Error("--ignore-case selects how --search compares letters: give --search too");
  if (a->show && a->search_args.empty())
    throw Error("--show N prints the lines a --search query returns: give --search too");
  if (a->tally && a->search_args.empty())
    throw Error("--tally K counts the words of the lines a --search query returns: give --search "
                "too (--top K is the same count over the whole text)");
  if (a->mark && !a->show)
    throw Error("--mark marks the matching tokens of the lines --show prints: give --show too");
  if (a->block_given && !a->index && a->search_args.empty())
    throw Error("--block-kb N builds the index of --index or --search block by block: give one of "
                "them too");
  if (a->keep_given && !a->block_given)
    throw Error("--keep-blocks M keeps the last M blocks of an index built block by block: give "
                "--block-kb N too");
  if (a->block_given && a->cfg.chunk_bytes)
    throw Error("--block-kb and --chunk-mb do not combine: --chunk-mb streams a word count, "
                "--block-kb builds an index block by block");
  if (a->index && !a->search_args.empty())
    throw Error("--index and --search do not combine: --index prints the whole index, "
                "--search the lines of its queries");
  if (a->index || !a->search_args.empty()) {
    // a search job is the index job plus the search stage: the same restrictions
    const std::string f = a->index ? "--index" : "--search";
    if (a->top)
      throw Error(f + " and --top do not combine: an index lists every word");
    if (a->cfg.ngram > 1)
      throw Error(f + " builds word keys only: not with --ngram N > 1");
    if (a->stage != 0 || !a->inputs.empty() || a->reducers > 1)
      throw Error(f + " runs whole jobs only: not with the stage split (stage 1 or 2, "
                  "--stage, --inputs, --reducer)");
    if (a->gpus > 1)
      throw Error(f + " runs on one GPU or the CPU: not with --gpus N > 1");
    if (a->cfg.chunk_bytes)
      throw Error(f + " takes one device pass: not with --chunk-mb (a streamed index is "
                  "not built; use --backend cpu for larger inputs, or --block-kb N to build "
                  "the index block by block)");
    if (!a->export_kiv.empty()) throw Error(f + " and --export-kiv do not combine");
    if (a->cfg.ref_timers) throw Error(f + " and --ref-timers do not combine");
    if (a->cfg.backend == Backend::kGpu && a->cfg.sort_path == SortPath::kRadix)
      throw Error(f + " on the GPU needs the dictionary path (--sort dict), not --sort radix");
    if (a->cfg.backend == Backend::kGpu && a->cfg.map_path == MapPath::kCompat)
      throw Error(f + " on the GPU needs the fast map (map_path fast), not --map-path "
                  "compat: the compat map overwrites the text the index reads again");
  }
  // the --search arguments, split with the job's own delimiter set: no term can be invalid
  const auto words = [&](const std::string& arg) {
    std::vector<std::string> terms;
    std::string cur;
    const auto delim = [&](char c) {
      // (--glob: a metacharacter is part of its word even when the job splits text at it)
      const bool meta = a->glob && (c == '*' || c == '?');
      return !meta && a->cfg.delimiters.find(c) != std::string::npos;
    };
    for (size_t i = 0; i < arg.size(); ++i) {
      const char c = arg[i];
      // (--regex: a word that begins with / runs to the next unescaped /, delimiters and blanks
      // included, and its closing slash ends the word)
      if (a->regex && c == '/' && cur.empty()) {
        size_t j = i + 1;
        while (j < arg.size() && arg[j] != '/') j += arg[j] == '\\' ? 2 : 1;
        if (j >= arg.size())
          throw Error("--search \"" + arg + "\": the regex term that starts at byte " +
                      std::to_string(i) + " has no closing /");
        if (j + 1 < arg.size() && !delim(arg[j + 1]))
          throw Error("--search \"" + arg + "\": the closing / of the regex term " +
                      arg.substr(i, j + 1 - i) + " must be followed by a delimiter or the end");
        terms.push_back(arg.substr(i, j + 1 - i));
        i = j;
        continue;
      }
      // (--fuzzy: so is a word's trailing ~d, the `~` and the digit)
      if (a->fuzzy && c == '~' && !cur.empty() && i + 1 < arg.size() && arg[i + 1] >= '0' &&
          arg[i + 1] <= '9' && (i + 2 == arg.size() || delim(arg[i + 2]))) {
        cur.push_back(c);
        cur.push_back(arg[++i]);
        continue;
      }
      if (delim(c)) {
        if (!cur.empty()) terms.push_back(cur);
        cur.clear();
      } else {
        cur.push_back(c);
      }
    }
    if (!cur.empty()) terms.push_back(cur);
    return terms;
  };
  for (size_t i = 0; i < a->search_args.size(); ++i) {
    const std::string& arg = a->search_args[i];
    if (a->match == "expr") {
      // the argument is the expression: split at blanks and parentheses only (make_search_expr),
      // so a term that holds a delimiter is refused, not cut in two
      if (!a->not_args[i].empty())
        throw Error("--not does not combine with --match expr: write NOT in the expression (\"" +
                    arg + " AND NOT ...\")");
      a->queries.push_back(make_search_expr(arg, a->cfg, a->wildcard, a->glob, a->fuzzy,
                                            a->regex));
      continue;
    }
    const SearchMode mode = a->match == "any"      ? SearchMode::kAny
                            : a->match == "phrase" ? SearchMode::kPhrase
                            : a->match == "near"   ? SearchMode::kNear
                                                   : SearchMode::kAll;
    const std::vector<std::string> terms = words(arg);
    if (terms.empty()) throw Error("--search \"" + arg + "\" holds no word");
    // (a --not that holds no word excludes nothing)
    const std::vector<std::string> exclude = words(a->not_args[i]);
    a->queries.push_back(make_search_query(terms, mode, a->wildcard, a->within, exclude, a->glob,
                                           a->fuzzy, a->regex));
  }
  // corpus: what --add does not go with, and the --in paths as file ids
  if (!a->add.empty()) {
    if (!a->index && a->search_args.empty())
      throw Error("--add FILE puts several files into one index: it goes with --index or "
                  "--search");
    if (a->window)
      throw Error("--add does not go with a line window: every file is indexed whole, and the "
                  "lines are numbered through the corpus");
  }
  if (a->by_file && a->search_args.empty())
    throw Error("--by-file and --count print a search's hits by file: give --search");
  for (size_t i = 0; i < a->queries.size(); ++i) {
    std::vector<std::string> paths{a->file};
    paths.insert(paths.end(), a->add.begin(), a->add.end());
    std::string cur;
    std::vector<u32> ids;
    const auto take = [&] {
      if (cur.empty()) return;
      const auto it = std::find(paths.begin(), paths.end(), cur);
      if (it == paths.end())
        throw Error("--in \"" + cur + "\" is none of the files given on the command line (the "
                    "input file and every --add FILE, spelt as there)");
      ids.push_back((u32)(it - paths.begin()));
      cur.clear();
    };
    for (const char c : a->in_args[i]) {
      if (c == ' ' || c == '\t')
        take();
      else
        cur.push_back(c);
    }
    take();
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    a->queries[i].files = ids;
  }
  if (!a->queries.empty()) {
    check_search_queries(a->queries, a->cfg);
    check_search_by_file(a->by_file, a->rank, a->show, a->tally);
    if (a->rank && (u64)a->cfg.emits_per_line > kRankMaxEmits)
      throw Error("--rank K takes --emits-per-line <= " + std::to_string(kRankMaxEmits) +
                  " (emits_per_line <= kRankMaxEmits: its scores fit 22 bits)");
    check_search_rank(a->rank, a->cfg, search_has_patterns(a->queries, a->ignore_case));
    if (a->cfg.backend == Backend::kGpu && a->queries.size() > (size_t)kSearchMaxQueries)
      throw Error("--search: a device batch holds at most " + std::to_string(kSearchMaxQueries) +
                  " queries (use --backend cpu for more)");
  }
  if (a->byte_range) {
    if (a->stage != 1) throw Error("--byte-range is a stage-1 (map) flag");
    a->window = false;  // the byte window replaces the positional line window
  }
  return true;
}

const char* spill_ext(SpillFormat f) {
  return f == SpillFormat::kBinary ? ".kv" : f == SpillFormat::kKiv ? ".kiv" : ".txt";
}
std::string spill_path(const CliArgs& a, int node) {
  return a.spill_dir + "/out." + std::to_string(node) + spill_ext(a.spill_fmt);
}
// Stage 2 without --inputs: this node's spill in the --spill-format named, else whichever
// of out.N.txt / .kv / .kiv exists (read_spill tells the formats apart by content).
std::string find_spill(const CliArgs& a, int node) {
  const std::string want = spill_path(a, node);
  if (access(want.c_str(), R_OK) == 0) return want;
  for (SpillFormat f : {SpillFormat::kText, SpillFormat::kBinary, SpillFormat::kKiv}) {
    const std::string p = a.spill_dir + "/out." + std::to_string(node) + spill_ext(f);
    if (access(p.c_str(), R_OK) == 0) return p;
  }
  return want;  // (its open fails with the path in the message)
}

// --json: one record per run, in every mode: counts, honest and
// reference-semantics stage times, and for --gpus N every rank's stage times and the bytes
// each of its links carried.
struct JsonOut {
  std::string body;
  void kv(const char* k, const std::string& raw) {
    body += (body.empty() ? "{" : ", ");
    body += "\"" + std::string(k) + "\": " + raw;
  }
  void num(const char* k, double v) {
    char b[64];
    std::snprintf(b, sizeof(b), "%.6f", v);
    kv(k, b);
  }
  void u(const char* k, unsigned long long v) { kv(k, std::to_string(v)); }
  void str(const char* k, const std::string& v) {
    std::string e;
    for (char c : v) {
      if ((unsigned char)c < 0x20) {  // control bytes (a TAB delimiter) as \u00XX
        char u[8];
        std::snprintf(u, sizeof(u), "\\u%04x", (unsigned)(unsigned char)c);
        e += u;
        continue;
      }
      if (c == '"' || c == '\\') e.push_back('\\');
      e.push_back(c);
    }
    kv(k, "\"" + e + "\"");
  }
  std::string done() const { return body + "}"; }
};

std::string u64_list(const std::vector<u64>& v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
  return s + "]";
}

void emit_json(const CliArgs& a, const std::string& text) {
  if (a.json.empty()) return;
  std::FILE* f = a.json == "-" ? stderr : std::fopen(a.json.c_str(), "w");
  if (!f) throw Error("cannot write json: " + a.json);
  std::fprintf(f, "%s\n", text.c_str());
  if (f != stderr) std::fclose(f);
}

JsonOut json_head(const CliArgs& a, const char* mode) {
  JsonOut j;
  j.str("mode", mode);
  j.str("backend", a.cfg.backend == Backend::kCpu ? "cpu" : "gpu");
  j.kv("gpus", std::to_string(a.gpus));
  j.str("map_path", to_string(a.cfg.map_path));
  j.str("reduce_path", to_string(a.cfg.reduce_path));
  j.str("sort", to_string(a.cfg.sort_path));
  j.u("ngram", (u64)a.cfg.ngram);
  return j;
}

void json_counts(JsonOut& j, const WordCountResult& r) {
  j.u("lines", r.num_lines);
  j.u("tokens", r.num_tokens);
  j.u("unique", r.num_unique);
  j.u("overflow_lines", r.overflow_lines);
  j.u("truncated", r.truncated);
  j.u("max_key_len", r.max_key_len);
}

// Where a one-shot single-GPU run's time goes, main() to the JSON line (run_direct):
// runtime init (the first HIP call), engine construction (code objects, device arena,
// pinned buffers), the file read, the first job, later jobs and the formatted output.
// Process start to main() (loader, static init) is the caller's wall clock minus these.
struct Startup {
  u64 main = 0, init = 0, engine = 0, read = 0, first = 0, jobs = 0, out = 0;
};
Startup g_startup;
const char* g_part_map = nullptr;  // "cache" / "default": run_direct's starting map

// The GPU engine's HBM plan (plan_device_pass): its device memory, the GPU's free and
// total memory before it, and whether the input streams (chunk size, map window).
GpuWordCount::Stats g_engine_stats;
bool g_engine_stats_set = false;
void json_hbm(JsonOut& j, const GpuWordCount::Stats& s) {
  j.u("hbm_device_bytes", s.device_bytes);
  j.u("hbm_free_bytes", s.hbm_free);
  j.u("hbm_total_bytes", s.hbm_total);
  j.kv("device_streaming", s.streaming ? "true" : "false");
  j.u("device_chunk_bytes", s.chunk_bytes);
  j.u("device_map_window", s.map_window);
}

// --top K: "top_k" in every mode's record, and where the device selected (one GPU) its
// device time and the bytes it wrote to host memory for the result.
const TopResult* g_top_device = nullptr;
void json_top(JsonOut& j, const CliArgs& a) {
  if (!a.top) return;
  j.u("top_k", a.top);
  if (g_top_device) {
    j.num("select_ms", g_top_device->select_ms);
    j.u("wire_bytes", g_top_device->wire_bytes);
  }
}

// --index: "index": true in the record, the postings' number, and where the device built
// it its device time and the bytes it wrote to host memory for the result.
// --block-kb: the blocks, the merges' device time (their sum) and the index store's size.
// --keep-blocks: the blocks dropped, the drops' device time (their sum) and the window's first
// line.
u64 g_blocks = 0, g_store_bytes = 0, g_dropped_blocks = 0, g_first_line = 0;
double g_append_ms = 0, g_drop_ms = 0;
void json_blocks(JsonOut& j, const CliArgs& a) {
  if (!a.block_given) return;
  j.u("blocks", g_blocks);
  j.num("append_ms", g_append_ms);
  j.u("index_store_bytes", g_store_bytes);
  if (!a.keep_given) return;
  j.u("dropped_blocks", g_dropped_blocks);
  j.num("drop_ms", g_drop_ms);
  j.u("first_line", g_first_line);
}

// corpus (--add): the resident files -- path, id, first_line, base, lines -- and the files the
// window has dropped.
u64 g_dropped_files = 0;
void json_files(JsonOut& j, const CliArgs& a, const std::vector<IndexSegment>& segs, u64 first,
                u64 lines) {
  if (a.add.empty()) return;
  IndexSegments t;
  t.reset(first, lines);
  if (!segs.empty()) t.segs = segs;
  std::string arr = "[";
  for (size_t i = 0; i < t.segs.size(); ++i) {
    const u32 id = t.segs[i].id;
    std::string path = id == 0 ? a.file : id <= a.add.size() ? a.add[id - 1] : std::string();
    std::string esc;
    for (const char c : path) {
      if (c == '"' || c == '\\') esc.push_back('\\');
      esc.push_back(c);
    }
    arr += std::string(i ? ", " : "") + "{\"path\": \"" + esc + "\", \"id\": " +
           std::to_string(id) + ", \"first_line\": " + std::to_string(t.segs[i].first_line) +
           ", \"base\": " + std::to_string(t.segs[i].base) + ", \"lines\": " +
           std::to_string(t.lines_of(i)) + "}";
  }
  j.kv("files", arr + "]");
  j.u("dropped_files", g_dropped_files);
}

const IndexResult* g_index = nullptr;
void json_index(JsonOut& j, const CliArgs& a) {
  if (!a.index) return;
  j.kv("index", "true");
  json_blocks(j, a);
  if (g_index) {
    j.num("index_ms", g_index->index_ms);
    j.u("postings", g_index->postings.size());
    j.u("wire_bytes", g_index->wire_bytes);
    json_files(j, a, g_index->segments, g_index->first_line, g_index->words.num_lines);
  }
}

// --search: "search": true in the record, the batch's size, its hits and the search time
// (the device stage's, or the host evaluation's), and the bytes the device wrote to host
// memory for the result.
const SearchResult* g_search = nullptr;
void json_search(JsonOut& j, const CliArgs& a) {
  if (a.queries.empty()) return;
  j.kv("search", "true");
  json_blocks(j, a);
  j.u("queries", a.queries.size());
  j.kv("regex", a.regex ? "true" : "false");
  if (g_search) {
    j.u("hits", g_search->lines.size());
    u64 matches = 0;
    for (const u64 m : g_search->matches) matches += m;
    j.u("rank_k", g_search->rank_k);
    j.u("matches", matches);
    j.num("index_ms", g_search->index_ms);
    j.num("search_ms", g_search->search_ms);
    j.u("show_bytes", g_search->show_bytes);
    j.num("show_ms", g_search->show_ms);
    j.u("cut_lines", g_search->cut_lines);
    j.u("spans", g_search->spans.size() / 3);
    j.u("tally", g_search->tally_k);
    j.num("tally_ms", g_search->tally_ms);
    j.u("tallied", g_search->tallied);
    j.u("wire_bytes", g_search->wire_bytes);
    j.u("merged", g_search->merged);
    j.u("walked", g_search->walked);
    j.u("restricted", g_search->restricted);
    json_files(j, a, g_search->segments, g_search->first_line, g_search->num_lines);
  }
}

// The statistics of a search result as a WordCountResult without entries.
WordCountResult search_stats(const SearchResult& t) {
  WordCountResult r;
  r.num_lines = t.num_lines;
  r.num_tokens = t.num_tokens;
  r.num_unique = t.num_unique;
  r.overflow_lines = t.overflow_lines;
  r.truncated = t.truncated;
  r.max_key_len = t.max_key_len;
  r.times = t.times;
  return r;
}

// The statistics of a top result as a WordCountResult without entries (json, timer lines).
WordCountResult top_stats(const TopResult& t) {
  WordCountResult r;
  r.num_lines = t.num_lines;
  r.num_tokens = t.num_tokens;
  r.num_unique = t.num_unique;
  r.overflow_lines = t.overflow_lines;
  r.truncated = t.truncated;
  r.max_key_len = t.max_key_len;
  r.chunks = t.chunks;
  r.times = t.times;
  return r;
}

void write_json(const CliArgs& a, const WordCountResult& r, const std::vector<double>& walls) {
  if (a.json.empty()) return;
  std::vector<double> w = walls;
  std::sort(w.begin(), w.end());
  const double med = w.empty() ? 0 : w[w.size() / 2];
  JsonOut j = json_head(a, "full");
  json_counts(j, r);
  j.num("map_ms", r.times.map_ms);
  j.num("process_ms", r.times.process_ms);
  j.num("reduce_ms", r.times.reduce_ms);
  j.num("h2d_ms", r.times.h2d_ms);
  j.num("d2h_ms", r.times.d2h_ms);
  j.num("ref_map_ms", r.times.ref_map_ms);
  j.num("ref_process_ms", r.times.ref_process_ms);
  j.num("ref_reduce_ms", r.times.ref_reduce_ms);
  j.num("wall_ms_median", med);
  j.kv("iters", std::to_string(w.size()));
  j.u("chunks", r.chunks);
  json_top(j, a);
  json_index(j, a);
  json_search(j, a);
  if (g_part_map) j.str("part_map", g_part_map);  // the one-shot CLI's starting map
  if (g_engine_stats_set) json_hbm(j, g_engine_stats);
  // peak resident memory of this process image (VmHWM: unlike getrusage's ru_maxrss it is
  // not inherited through the fork + exec that started us)
  j.u("max_rss_kb", peak_rss_kb());
  if (g_startup.init) {
    const Startup& t = g_startup;
    const u64 end = now_ns();
    auto ms = [](u64 a0, u64 a1) { return a1 > a0 ? (a1 - a0) * 1e-6 : 0.0; };
    JsonOut st;
    st.num("runtime_init_ms", ms(t.main, t.init));
    st.num("engine_ms", ms(t.init, t.engine));
    st.num("read_ms", ms(t.engine, t.read));
    st.num("first_job_ms", ms(t.read, t.first));
    st.num("later_jobs_ms", ms(t.first, t.jobs));
    st.num("output_ms", ms(t.jobs, end));
    st.num("main_to_json_ms", ms(t.main, end));
    // before main(): the loader and the libraries' static initialisation, split at this
    // library's own (LOCUST_T0: the spawner's CLOCK_MONOTONIC ns, tools/cli_cold.py)
    st.num("library_to_main_ms", ms(library_init_ns(), t.main));
    if (const char* t0 = std::getenv("LOCUST_T0"))
      st.num("spawn_to_library_ms", ms((u64)std::strtoull(t0, nullptr, 10), library_init_ns()));
    j.kv("startup", st.done());
  }
  emit_json(a, j.done());
}

void write_json_dist(const CliArgs& a, const DistResult& root, const std::vector<DistResult>& ranks) {
  if (a.json.empty()) return;
  JsonOut j = json_head(a, "multi_gpu");
  json_counts(j, root.result);
  j.str("strategy", root.strategy == DistStrategy::kGather    ? "gather"
                    : root.strategy == DistStrategy::kLocal   ? "local"
                                                              : "shuffle");
  j.num("wall_ms", root.total_ms);
  json_top(j, a);
  j.str("comm", !ranks.empty() && ranks[0].rccl_clique ? "rccl" : "loopback");
  j.u("peak_rss_kb", peak_rss_kb());
  {  // page-locked host memory: every rank's engine, plus the shared output block once
    u64 pinned = ranks.empty() ? 0 : ranks[0].shared_pinned_bytes;
    for (const DistResult& d : ranks) pinned += d.pinned_bytes;
    j.u("pinned_bytes", pinned);
    u64 hbm = 0;
    for (const DistResult& d : ranks) hbm += d.hbm_device_bytes;
    j.u("hbm_device_bytes", hbm);  // every rank's engines (one GPU or several)
    if (!ranks.empty()) j.u("hbm_total_bytes", ranks[0].hbm_total_bytes);
    u64 used = 0;
    for (const DistResult& d : ranks) used = std::max(used, d.hbm_used_bytes);
    j.u("hbm_used_bytes_max", used);
  }
  std::string rk = "[";
  for (size_t r = 0; r < ranks.size(); ++r) {
    const DistResult& d = ranks[r];
    JsonOut x;
    x.kv("rank", std::to_string(r));
    x.num("map_ms", d.map_ms);
    x.num("shuffle_ms", d.shuffle_ms);
    x.num("reduce_ms", d.reduce_ms);
    x.num("gather_ms", d.gather_ms);
    x.num("total_ms", d.total_ms);
    x.u("local_records", d.local_records);
    x.u("range_tokens", d.range_tokens);
    x.u("range_unique", d.range_unique);
    x.u("sent_bytes", d.sent_bytes);
    x.u("recv_bytes", d.recv_bytes);
    x.kv("sent_to", u64_list(d.sent_to));
    x.kv("recv_from", u64_list(d.recv_from));
    x.u("output_bytes", d.output_bytes);
    x.kv("device_exchange", d.device_exchange ? "true" : "false");
    x.u("host_syncs", (u64)d.host_syncs);
    x.u("input_bytes", d.input_bytes);
    x.kv("input_streamed", d.input_streamed ? "true" : "false");
    x.kv("peer_p2p", std::to_string(d.peer_p2p));
    x.u("pinned_bytes", d.pinned_bytes);
    x.u("hbm_device_bytes", d.hbm_device_bytes);
    x.u("hbm_free_bytes", d.hbm_free_bytes);
    x.u("hbm_total_bytes", d.hbm_total_bytes);
    x.u("hbm_used_bytes", d.hbm_used_bytes);
    rk += (r ? ", " : "") + x.done();
  }
  j.kv("ranks", rk + "]");
  emit_json(a, j.done());
}

long long ns(double ms) { return (long long)(ms * 1e6 + 0.5); }

// Writes the synthetic text in 64 MiB pieces (bounded memory for 10 GB files).
int generate(const CliArgs& a) {
  std::FILE* f = std::fopen(a.gen_out.c_str(), "wb");
  if (!f) throw Error("cannot write " + a.gen_out);
  const u64 piece_lines = 1u << 20;  // whole 1,024-line blocks per piece
  u64 lines = 0, bytes = 0;
  std::string buf;
  for (u64 first = 0;; first += piece_lines / kGenBlockLines) {
    GenSpec g = a.gen;
    g.first_block = first;
    if (a.gen.lines) {
      if (lines >= a.gen.lines) break;
      g.lines = std::min<u64>(piece_lines, a.gen.lines - lines);
      g.bytes = 0;
    } else {
      if (bytes >= a.gen.bytes) break;
      g.lines = std::min<u64>(piece_lines, a.gen.bytes);  // cut below by bytes
    }
    buf.clear();
    u64 nl = gen_text(g, &buf);
    if (!a.gen.lines && bytes + buf.size() > a.gen.bytes) {
      const size_t cut = buf.rfind('\n', a.gen.bytes - bytes - 1);
      if (cut == std::string::npos || a.gen.bytes == bytes) break;
      buf.resize(cut + 1);
      nl = count_newlines(buf.data(), buf.size());
    }
    write_all(f, buf);
    lines += nl;
    bytes += buf.size();
    if (!a.gen.lines && nl < piece_lines) break;
  }
  std::fclose(f);
  std::printf("generated %llu lines, %llu bytes -> %s\n", (unsigned long long)lines,
              (unsigned long long)bytes, a.gen_out.c_str());
  return 0;
}

// The result lines: the GPU build's "print key: k \t val: v \t count: c" (main.cu:132) or
// the CPU build's "print key: k \t value: c" (main.cu:286).  By default the backend's own
// build -- except --gpus N, always the GPU build's (the multi-GPU mode; --backend cpu there
// only rehearses its ranks, docs/PARITY.md) -- and --output-format overrides.
void format_results(const CliArgs& a, bool cpu_default, const WordCountResult& r,
                    std::string* out) {
  if (a.quiet) return;
  const bool cpu = a.out_format ? a.out_format == 2 : cpu_default;
  (cpu ? format_cpu_output : format_gpu_output)(r, out);
}

// --top K: the same lines for the K winners only, in rank order.
void format_top(const CliArgs& a, bool cpu_default, const TopResult& t, std::string* out) {
  if (a.quiet) return;
  const bool cpu = a.out_format ? a.out_format == 2 : cpu_default;
  format_top_output(t, cpu, out);
}
// ... selected on the host from a complete result (multi-rank jobs, stage 2, the CPU).
void format_results_or_top(const CliArgs& a, bool cpu_default, const WordCountResult& r,
                           std::string* out) {
  if (a.top)
    format_top(a, cpu_default, top_result(r, a.top), out);
  else
    format_results(a, cpu_default, r, out);
}

// The result lines to stdout, or to --result-file (a range reducer on a worker daemon,
// whose reply carries only the tail of stdout).
// --by-file / --count: format_search_output's lines with, under each query's line and above its
// shown and tally lines, one line per file of the query's CSR:
//   "  file: <path> \t hits: <n> \t lines: <local> <local> ...\n"
// (ranked: "top:" and <local>:<score>, in rank order; --count: the line ends behind its hits,
// and the query's line ends behind "hits: <n>" with " \t files: <f>").  With --show a shown
// line's prefix becomes "<path>:<local>: ".
void format_search_by_file(const CliArgs& a, const SearchResult& r, std::string* out) {
  std::string plain;
  format_search_output(r, &plain, a.mark);
  if (r.by_file == kByFileNone) {
    out->append(plain);
    return;
  }
  const auto path_of = [&](u32 id) {
    return id == 0 ? a.file : id <= a.add.size() ? a.add[id - 1] : "file " + std::to_string(id);
  };
  const bool count = r.by_file == kByFileCount;
  size_t at = 0, q = 0;
  u64 shown = 0;  // entries of query q - 1 whose shown line is still to come
  u64 entry = 0;
  while (at < plain.size()) {
    size_t nl = plain.find('\n', at);
    if (nl == std::string::npos) nl = plain.size();
    std::string line = plain.substr(at, nl - at);
    at = nl + 1;
    if (line.compare(0, 12, "print query:") == 0 && q < r.queries.size()) {
      const u64 f0 = r.file_off[q], f1 = r.file_off[q + 1];
      if (count) {
        const size_t cut = line.find(" \t hits: ");
        if (cut != std::string::npos) {
          // (the lines stay on the device: the hits are the matches)
          line = line.substr(0, cut) + " \t hits: " + std::to_string(r.matches[q]);
        }
        line += " \t files: " + std::to_string(f1 - f0);
      }
      out->append(line + "\n");
      for (u64 f = f0; f < f1; ++f) {
        out->append("  file: " + path_of(r.file_ids[f]) + " \t hits: " +
                    std::to_string(r.file_counts[f]));
        if (!count) {
          out->append(r.rank_k ? " \t top:" : " \t lines:");
          for (u64 j = r.offsets[q]; j < r.offsets[q + 1]; ++j) {
            if (r.line_file[j] != r.file_ids[f]) continue;
            out->append(" " + std::to_string(r.line_local[j]));
            if (r.rank_k) out->append(":" + std::to_string(r.scores[j]));
          }
        }
        out->push_back('\n');
      }
      entry = count ? 0 : r.offsets[q];
      shown = r.show_bytes && !count ? r.offsets[q + 1] - r.offsets[q] : 0;
      ++q;
      continue;
    }
    if (shown && line.compare(0, 2, "  ") == 0) {  // "  <global>: <bytes>" -> "  <path>:<local>: "
      const size_t colon = line.find(": ", 2);
      if (colon != std::string::npos)
        line = "  " + path_of(r.line_file[entry]) + ":" + std::to_string(r.line_local[entry]) +
               line.substr(colon);
      ++entry;
      --shown;
    }
    out->append(line + "\n");
  }
}

void emit_results(const CliArgs& a, const std::string& out) {
  if (a.result_file.empty()) {
    std::fflush(stdout);
    write_all(stdout, out);
    return;
  }
  std::FILE* f = std::fopen(a.result_file.c_str(), "wb");
  if (!f) throw Error("cannot write " + a.result_file);
  write_all(f, out);
  if (std::fclose(f) != 0) throw Error("error closing " + a.result_file);
}

// `top` (--top K on one GPU): the device selected; r then carries the statistics only.
// `idx` (--index): the result lines are the index's.  `srch` (--search): the queries'.
void print_gpu_result(const CliArgs& a, const WordCountResult& r, const std::vector<double>& walls,
                      const TopResult* top = nullptr, const IndexResult* idx = nullptr,
                      const SearchResult* srch = nullptr) {
  const bool rt = a.cfg.ref_timers;
  std::printf("GPU mapping %lld nanoseconds \n", ns(rt ? r.times.ref_map_ms : r.times.map_ms));
  for (u64 k = 0; k < r.overflow_lines; ++k) std::printf("WARN: Exceeded emit limit\n");
  std::printf("GPU stream compaction and sorting %lld nanoseconds \n",
              ns(rt ? r.times.ref_process_ms : r.times.process_ms));
  std::printf("GPU reduce %lld nanoseconds \n", ns(rt ? r.times.ref_reduce_ms : r.times.reduce_ms));
  if (r.truncated)
    LOCUST_LOG_WARN("%llu tokens longer than %d chars were truncated",
                    (unsigned long long)r.truncated, a.cfg.max_key_len);
  std::string out;
  if (srch) {
    if (!a.quiet) format_search_by_file(a, *srch, &out);
  } else if (idx) {
    if (!a.quiet) format_index_output(*idx, &out);
  } else if (top) {
    format_top(a, false, *top, &out);
  } else {
    format_results(a, false, r, &out);
  }
  emit_results(a, out);
  std::fflush(stdout);
  g_top_device = top;
  g_index = idx;
  g_search = srch;
  write_json(a, r, walls);
  if (!a.export_kiv.empty()) write_kiv_results(a.export_kiv, r);
  std::printf("\nDone\n");
}

// Peak resident host memory (kB, VmHWM of /proc/self/status).
unsigned long long peak_rss_kb() {
  std::FILE* f = std::fopen("/proc/self/status", "r");
  if (!f) return 0;
  char line[256];
  unsigned long long kb = 0;
  while (std::fgets(line, sizeof(line), f))
    if (std::sscanf(line, "VmHWM: %llu kB", &kb) == 1) break;
  std::fclose(f);
  return kb;
}

// Stream threshold: files past one device pass (--chunk-mb, default 256 MiB) stream.
constexpr u64 kDefaultStreamChunk = 256ull << 20;

// The RSS stamps of --json runs at LOCUST_LOG=info (reading /proc costs the one-shot CLI).
void log_rss(const char* when) {
  if ((int)log_level() >= (int)LogLevel::kInfo)
    LOCUST_LOG_INFO("%s: %s", when, process_rss_breakdown().c_str());
}

int run_direct(const CliArgs& a) {
  JobConfig cfg = a.cfg;
  const u64 size = file_size(a.file);
  const u64 chunk = cfg.chunk_bytes ? cfg.chunk_bytes : kDefaultStreamChunk;
  WordCountResult r;
  TopResult top;  // --top K: selected on the device, r keeps the statistics
  std::vector<double> walls;
  log_rss("before the engine");
  Startup& st = g_startup;
  (void)visible_device_count();  // the HIP runtime's own start-up, timed apart
  st.init = now_ns();
  // The engine outlives the output: its teardown (stream, pinned buffers) is not a job's
  std::unique_ptr<GpuWordCount> eng;
  // the partition map tuned by an earlier run on this file (io.hpp partition-map cache)
  const std::string pmc = partmap_cache_path(a.file, cfg);
  std::vector<u64> cached;
  auto start_map = [&]() {
    g_part_map = load_partmap_cache(pmc, &cached) && eng->set_partition_map(cached) ? "cache"
                                                                                    : "default";
  };
  if (size > chunk) {
    cfg.chunk_bytes = chunk;
    eng.reset(new GpuWordCount(cfg, size, size));
    g_engine_stats = eng->stats();
    g_engine_stats_set = true;
    start_map();
    st.engine = st.read = now_ns();  // the file is read by the job, piece by piece
    log_rss("with the streaming engine");
    for (int i = 0; i < a.warmup + a.iters; ++i) {
      auto src = open_file_source(a.file);
      if (a.top) {
        top = eng->run_top_source(*src, (u32)std::min<u64>(a.top, 0xFFFFFFFFu));
        r = top_stats(top);
      } else {
        r = eng->run_source(*src);
      }
      if (i >= a.warmup) walls.push_back(r.times.wall_ms);
      if (i == 0) st.first = now_ns();
    }
  } else {
    eng.reset(new GpuWordCount(cfg, std::max<u64>(size, 1), std::max<u64>(size, 1)));
    g_engine_stats = eng->stats();
    g_engine_stats_set = true;
    start_map();
    st.engine = now_ns();
    TextInput in;
    in.data = eng->input_buffer();
    in.bytes = read_file_into(a.file, eng->input_buffer(), std::max<u64>(size, 1), &in.num_lines);
    in.first_line = 0;
    st.read = now_ns();
    std::vector<u64> stamps;  // per job: start, after run(), after the result is stored
    stamps.reserve(3 * (size_t)(a.warmup + a.iters));
    std::vector<StageTimes> jt;  // per job: its own host split (launch / wait / copy)
    jt.reserve((size_t)(a.warmup + a.iters));
    for (int i = 0; i < a.warmup + a.iters; ++i) {
      stamps.push_back(now_ns());
      if (a.top) {
        top = eng->run_top(in, (u32)std::min<u64>(a.top, 0xFFFFFFFFu));
        stamps.push_back(now_ns());
        jt.push_back(top.times);
        r = top_stats(top);
        if (i >= a.warmup) walls.push_back(r.times.wall_ms);
      } else if (i < a.warmup) {
        jt.push_back(eng->run(in).times);
        stamps.push_back(now_ns());
      } else {
        WordCountResult x = eng->run(in);
        stamps.push_back(now_ns());
        jt.push_back(x.times);
        r = std::move(x);
        walls.push_back(r.times.wall_ms);
      }
      stamps.push_back(now_ns());
      if (i == 0) st.first = stamps.back();
    }
    if ((int)log_level() >= (int)LogLevel::kDebug)
      for (size_t k = 0; k + 2 < stamps.size(); k += 3)
        LOCUST_LOG_DEBUG("job %zu: starts %+.3f ms, run() %.3f ms (launch %.3f, wait %.3f, copy "
                         "%.3f), result stored %.3f ms", k / 3, (stamps[k] - st.read) * 1e-6,
                         (stamps[k + 1] - stamps[k]) * 1e-6, jt[k / 3].host_launch_ms,
                         jt[k / 3].host_wait_ms, jt[k / 3].host_copy_ms,
                         (stamps[k + 2] - stamps[k + 1]) * 1e-6);
    r.num_lines = in.num_lines;
  }
  st.jobs = now_ns();
  log_rss("after the job");
  std::printf("Length: %i\n", (int)r.num_lines);
  print_gpu_result(a, r, walls, a.top ? &top : nullptr);
  log_rss("after the output");
  // keep this run's tuned map for the next run on the file (after the output: not a job's)
  const u64 t_down = now_ns();
  std::vector<u64> lo;
  if (!pmc.empty() && eng->partition_map(&lo) && lo != cached) save_partmap_cache(pmc, lo);
  if (fast_exit_ok()) {
    // the process ends right after this (main: _exit): the driver reclaims the engine's
    // queues and memory with the process -- no per-buffer teardown
    (void)eng.release();
    g_fast_exit = true;
    return 0;
  }
  eng.reset();
  LOCUST_LOG_DEBUG("engine teardown %.3f ms", (now_ns() - t_down) * 1e-6);
  return 0;
}

// ---------------- stage 1: map only -> spill (main.cu:421-433) ----------------
// The combined map output -- one (key, count) record per distinct key, in key order -- and
// its index.  A GPU line window is found by a newline scan and read straight from the file
// into the engine's pinned buffer; past one device pass (--chunk-mb, 256 MiB) it streams
// through a streaming engine, so host memory stays bounded for any window size.
// --ref-compat keeps the reference's spill: one "key \t1" record per token, sorted.
int run_map_stage(const CliArgs& a) {
  const bool cpu = a.cfg.backend == Backend::kCpu;
  const char* dev = cpu ? "CPU" : "GPU";
  const std::string path = spill_path(a, a.node);
  // the HIP runtime's own start-up (once per process, ~0.1-0.2 s), timed apart from the
  // job like run_direct's: job_ms is this window's work, comparable across processes
  const u64 t_init = now_ns();
  if (!cpu) (void)visible_device_count();
  const double runtime_init_ms = (now_ns() - t_init) * 1e-6;
  MapWindow win;
  if (a.byte_range) {
    win.by_bytes = true;
    win.byte_begin = a.byte_begin;
    win.byte_end = a.byte_end;
  } else if (a.window) {
    win.line_start = a.line_start;
    win.line_end = a.line_end;
  }
  MapStageResult m = map_stage(a.cfg, a.file, win, path, a.spill_fmt);
  if (m.engine_keep && fast_exit_ok()) {  // main _exits after the output: no teardown
    new std::shared_ptr<void>(std::move(m.engine_keep));  // never destroyed
    g_fast_exit = true;
  }
  const WordCountResult& r = m.result;
  if (!cpu) std::printf("Length: %i\n", (int)m.lines);
  for (u64 k = 0; k < r.overflow_lines; ++k) std::printf("WARN: Exceeded emit limit\n");
  // event-timed on the GPU: H2D + map, then compaction/combine + sort
  std::printf("%s mapping %lld nanoseconds \n", dev, ns(r.times.h2d_ms + r.times.map_ms));
  std::printf("%s stream compaction and sorting %lld nanoseconds \n", dev,
              ns(r.times.process_ms + r.times.reduce_ms));
  if (!a.json.empty()) {
    JsonOut j = json_head(a, "map_stage");
    json_counts(j, r);
    j.u("spill_records", m.spill_records);
    j.u("spill_bytes", m.index.spill_bytes);
    j.str("spill", path);
    j.str("input", a.file);
    j.kv("line_start", std::to_string(a.window ? a.line_start : 0));
    j.kv("line_end", std::to_string(a.window ? a.line_end : -1));
    if (a.byte_range) {  // the range asked for, and the bytes it moved to
      j.u("byte_range_begin", a.byte_begin);
      j.kv("byte_range_end", a.byte_end == ~0ull ? "-1" : std::to_string(a.byte_end));
    }
    j.u("byte_begin", m.byte_begin);
    j.u("byte_end", m.byte_end);
    {  // the input's identity and the tokenizer settings (a resume checks both)
      struct stat st {};
      if (::stat(a.file.c_str(), &st) == 0) {
        j.u("input_size", (unsigned long long)st.st_size);
        j.u("input_mtime_ns", (unsigned long long)st.st_mtim.tv_sec * 1000000000ull +
                                  (unsigned long long)st.st_mtim.tv_nsec);
        j.u("input_inode", (unsigned long long)st.st_ino);
      }
      j.kv("emits_per_line", std::to_string(a.cfg.emits_per_line));
      j.kv("max_key", std::to_string(a.cfg.max_key_len));
      j.str("delimiters", a.cfg.delimiters);
    }
    j.kv("combined", a.cfg.ref_compat ? "false" : "true");
    j.kv("streamed", m.streamed ? "true" : "false");
    j.u("input_bytes", m.input_bytes);
    j.num("map_ms", r.times.h2d_ms + r.times.map_ms);
    j.num("process_ms", r.times.process_ms + r.times.reduce_ms);
    j.num("job_ms", m.job_ms);
    j.num("runtime_init_ms", runtime_init_ms);
    j.num("window_ms", m.window_ms);
    j.num("setup_ms", m.setup_ms);
    j.num("run_ms", m.run_ms);
    j.num("spill_write_ms", m.spill_write_ms);
    if (!cpu && !a.cfg.ref_compat) json_hbm(j, m.engine);
    j.u("peak_rss_kb", peak_rss_kb());
    emit_json(a, j.done());
  }
  std::printf("MODE_MULTI: Finished map\n");
  return 0;
}

// ---------------- stage 2: reduce only (main.cu:437-486) ----------------
// Every spill is a sorted run (the reference's reducer needed one pre-sorted file, B7):
// this reducer's key range of each is read (an index seek) and merged, counts summed --
// never expanded into tokens.  --reducer r/R: key range r of R, with its global val base.
int run_reduce_stage(const CliArgs& a) {
  const bool cpu = a.cfg.backend == Backend::kCpu;
  std::vector<std::string> files = a.inputs;
  if (files.empty()) files.push_back(find_spill(a, a.node));
  const u64 t_init = now_ns();  // the HIP runtime's start-up, apart from setup_ms
  if (!cpu) (void)visible_device_count();
  const double runtime_init_ms = (now_ns() - t_init) * 1e-6;
  ReduceStageStats st;
  WordCountResult r = reduce_spills(a.cfg, files, a.reducer, a.reducers, &st);
  std::printf("%s reduce %lld nanoseconds \n", cpu ? "CPU" : "GPU", ns(st.merge_ms));
  std::string out;
  format_results_or_top(a, cpu, r, &out);  // --top: of this reducer's key range
  emit_results(a, out);
  if (!a.json.empty()) {
    JsonOut j = json_head(a, "reduce_stage");
    json_counts(j, r);
    json_top(j, a);
    j.u("input_files", st.input_files);
    j.u("indexed_files", st.indexed_files);
    j.u("records_read", st.records_read);
    j.u("input_records", st.run_records);
    j.kv("reducer", std::to_string(a.reducer));
    j.kv("reducers", std::to_string(a.reducers));
    j.u("val_base", r.val_base);
    j.num("read_ms", st.read_ms);
    j.num("runtime_init_ms", runtime_init_ms);
    j.num("setup_ms", st.setup_ms);
    j.num("merge_ms", st.merge_ms);
    j.num("wall_ms", r.times.wall_ms);
    j.u("peak_rss_kb", peak_rss_kb());
    emit_json(a, j.done());
  }
  if (!a.export_kiv.empty()) write_kiv_results(a.export_kiv, r);
  std::printf("\nDone\n");
  return 0;
}

int run(const CliArgs& a) {
  if (!a.gen_out.empty()) return generate(a);
  const bool cpu = a.cfg.backend == Backend::kCpu;
  const char* dev = cpu ? "CPU" : "GPU";
  if (a.window)
    std::printf("Using custom start and end locations: (%i, %i)\n", (int)a.line_start,
                (int)a.line_end);

  if (a.stage == 2) return run_reduce_stage(a);
  if (a.stage == 1) return run_map_stage(a);

  // CPU build ignores the line window (its loadFile takes none, main.cu:242) -- only
  // reproduced under --ref-compat.
  const bool use_window = a.window && !(cpu && a.cfg.ref_compat);
  // A whole file on one GPU (the fast dictionary path): no loader copy at all -- the file
  // is read by parallel preads straight into the engine's pinned input buffer, or, past
  // one device pass, streamed through two pinned chunks (host memory stays bounded).
  const bool direct = !cpu && !use_window && a.stage == 0 && !a.gpus_given && a.gpus <= 1 &&
                      !a.cfg.ref_compat && a.cfg.map_path == MapPath::kFast &&
                      a.cfg.sort_path == SortPath::kDict && !a.index && a.queries.empty();
  if (direct) return run_direct(a);
  // ---------------- multi-GPU in one process (one thread per rank) ----------------------
  // An explicit --gpus N (N >= 1) runs N ranks.  --comm auto: an ncclCommInitAll clique
  // over xGMI when N > 1 and every rank has a GPU of its own, loopback ranks otherwise
  // (one rank, or N ranks rehearsed on fewer GPUs); --comm rccl / loopback force either.
  // A whole file is never loaded: every rank reads only its own line-aligned byte range
  // (run_single_process_file); a line window is loaded first, then sharded.
  const bool multi = (a.gpus > 1 || (a.gpus_given && !cpu)) && a.stage == 0 && !a.index &&
                     a.queries.empty();
  // (the compat map sizes its slots per line: its ranks get the loaded text, whose line
  // count is exact, not a file range sized by bytes)
  const bool file_ranks = multi && !use_window && !a.cfg.ref_compat &&
                          a.cfg.map_path != MapPath::kCompat;
  LoadedText text;
  if (!file_ranks) {
    text = load_lines(a.file, use_window ? a.line_start : -1, use_window ? a.line_end : -1,
                      a.cfg.ref_compat);
    if (!cpu) std::printf("Length: %i\n", (int)text.input.num_lines);
  }
  if (multi) {
    DistConfig dc;
    dc.job = a.cfg;
    // ranks always combine map-side (the output is the same; the device exchange and the
    // gather slots move one record per distinct key instead of one per token)
    dc.job.combine = true;
    dc.world = std::max(1, a.gpus);
    dc.strategy = a.strategy;
    std::vector<DistResult> ranks;
    DistResult dr = file_ranks ? run_single_process_file(dc, a.file, a.comm, &ranks)
                               : run_single_process_multi_gpu(dc, text.input, a.comm, &ranks);
    // the communicator the ranks actually used (a failed clique falls back to loopback)
    LOCUST_LOG_INFO("%d ranks in one process over %s", dc.world,
                    !ranks.empty() && ranks[0].rccl_clique ? "an RCCL clique" : "loopback");
    log_rss("after the job");
    if (file_ranks && !cpu) std::printf("Length: %i\n", (int)dr.result.num_lines);
    std::printf("%s mapping %lld nanoseconds \n", dev, ns(dr.map_ms));
    std::printf("%s stream compaction and sorting %lld nanoseconds \n", dev, ns(dr.shuffle_ms));
    std::printf("%s reduce %lld nanoseconds \n", dev, ns(dr.reduce_ms));
    std::string out;
    format_results_or_top(a, false, dr.result, &out);
    emit_results(a, out);
    write_json_dist(a, dr, ranks);
    std::printf("\nDone\n");
    return 0;
  }

  // ---------------- corpus: the --add files behind the first, in one buffer ----------------
  // A file that lacks its last newline gets one when another follows (the byte makes no new
  // line).  Every file begins a segment of the index; --block-kb cuts each file on its own.
  std::vector<char> corpus;
  std::vector<TextInput> corpus_files;
  if (!a.add.empty()) {
    std::vector<std::pair<u64, u64>> parts;  // (bytes, lines) per file
    const auto put = [&](const TextInput& in, bool last) {
      corpus.insert(corpus.end(), in.data, in.data + in.bytes);
      if (!last && in.bytes && in.data[in.bytes - 1] != '\n') corpus.push_back('\n');
      parts.emplace_back(in.bytes + (!last && in.bytes && in.data[in.bytes - 1] != '\n'),
                         in.num_lines);
    };
    put(text.input, false);
    for (size_t i = 0; i < a.add.size(); ++i)
      put(load_lines(a.add[i], -1, -1, a.cfg.ref_compat).input, i + 1 == a.add.size());
    u64 off = 0, line = 0;
    for (const auto& p : parts) {
      TextInput in;
      in.data = corpus.data() + off;
      in.bytes = p.first;
      in.num_lines = p.second;
      in.first_line = line;
      corpus_files.push_back(in);
      off += p.first;
      line += p.second;
    }
    text.input = TextInput{};
    text.input.data = corpus.data();
    text.input.bytes = off;
    text.input.num_lines = line;
  }
  const bool blocked = a.block_given || !a.add.empty();
  std::vector<char> new_file;  // parallel to the blocks: the block begins a file
  const auto make_blocks = [&] {
    std::vector<TextInput> out;
    new_file.clear();
    if (corpus_files.empty()) {
      out = split_blocks(text.input, a.block_kb << 10);
      new_file.assign(out.size(), 0);
      return out;
    }
    for (size_t f = 0; f < corpus_files.size(); ++f) {
      const std::vector<TextInput> bs = a.block_given
                                            ? split_blocks(corpus_files[f], a.block_kb << 10)
                                            : std::vector<TextInput>{corpus_files[f]};
      for (size_t j = 0; j < bs.size(); ++j) {
        out.push_back(bs[j]);
        new_file.push_back(f > 0 && j == 0);
      }
    }
    return out;
  };
  g_dropped_files = 0;

  // ---------------- stage 0: full pipeline ----------------
  WordCountResult r;
  TopResult cpu_top;  // --top K on the CPU backend
  IndexResult cpu_index;  // --index on the CPU backend
  SearchResult cpu_search;  // --search on the CPU backend
  std::vector<double> walls;
  if (cpu) {
    CpuWordCount eng(a.cfg);
    for (int i = 0; i < a.warmup; ++i) eng.run(text.input);
    for (int i = 0; i < a.iters; ++i) {
      if (blocked) {
        // per block an index of its own, joined on the host (merge_index); a search then runs
        // over the merged index and the whole text
        const u64 t0 = now_ns();
        const std::vector<TextInput> blocks = make_blocks();
        g_dropped_files = 0;
        IndexResult x = eng.run_index(blocks[0]);
        // --keep-blocks: the dropped lines' statistics come from each block's own index
        std::vector<std::pair<u64, u64>> stats{{x.words.overflow_lines, x.words.truncated}};
        size_t oldest = 0;  // the first block still in the index
        for (size_t b = 1; b < blocks.size(); ++b) {
          const IndexResult y = eng.run_index(blocks[b]);
          StageTimes tm = x.words.times;
          tm.map_ms += y.words.times.map_ms;
          tm.process_ms += y.words.times.process_ms;
          tm.reduce_ms += y.words.times.reduce_ms;
          stats.emplace_back(y.words.overflow_lines, y.words.truncated);
          x = merge_index(x, y, new_file[b] != 0);
          if (a.keep_given && b + 1 - oldest > a.keep_blocks) {
            g_dropped_files += x.segment_table().drop(blocks[oldest].num_lines);
            x = trim_index(x, blocks[oldest].num_lines, stats[oldest].first, stats[oldest].second);
            ++oldest;
          }
          x.words.times = tm;
        }
        g_blocks = blocks.size();
        g_dropped_blocks = oldest;
        g_first_line = x.first_line;
        TextInput window = text.input;  // the lines still in the index
        window.data = blocks[oldest].data;
        window.bytes = (u64)(text.input.data + text.input.bytes - window.data);
        window.first_line = blocks[oldest].first_line;
        window.num_lines = text.input.first_line + text.input.num_lines - window.first_line;
        if (!a.queries.empty()) {
          cpu_search = search_index(x, window, a.queries, a.cfg, a.rank, a.ignore_case,
                                    a.show, a.tally, a.by_file);
          r = search_stats(cpu_search);
          r.times = x.words.times;
        } else {
          cpu_index = std::move(x);
          r = cpu_index.words;
        }
        r.times.wall_ms = (now_ns() - t0) * 1e-6;
      } else if (!a.queries.empty()) {
        cpu_search =
            eng.run_search(text.input, a.queries, a.rank, a.ignore_case, a.show, a.tally,
                           a.by_file);
        r = search_stats(cpu_search);
      } else if (a.index) {
        cpu_index = eng.run_index(text.input);
        r = cpu_index.words;
      } else if (a.top) {
        cpu_top = eng.run_top(text.input, a.top);
        r = top_stats(cpu_top);
      } else {
        r = eng.run(text.input);
      }
      walls.push_back(r.times.wall_ms);
    }
    std::printf("CPU mapping %lld nanoseconds \n", ns(r.times.map_ms));
    std::printf("CPU sorting %lld nanoseconds \n", ns(r.times.process_ms));
    std::printf("CPU reducing %lld nanoseconds \n", ns(r.times.reduce_ms));
  } else {
    if (blocked) {
      // the first block indexed, the rest appended on the device; the engine holds one block
      const std::vector<TextInput> blocks = make_blocks();
      u64 max_bytes = 1, max_lines = 1;
      for (const TextInput& b : blocks) {
        max_bytes = std::max(max_bytes, b.bytes);
        max_lines = std::max(max_lines, b.num_lines);
      }
      GpuWordCount eng(a.cfg, max_bytes, max_lines);
      IndexResult x;
      SearchResult sr;
      for (int i = 0; i < a.warmup + a.iters; ++i) {
        const u64 t0 = now_ns();
        StageTimes tm = eng.run_index(blocks[0]).words.times;
        double index_ms = 0, append_ms = 0, drop_ms = 0;
        size_t oldest = 0;  // the first block still in the index
        u64 first_line = blocks[0].first_line;
        g_dropped_files = 0;
        for (size_t b = 1; b < blocks.size(); ++b) {
          const IndexAppend ap = eng.append_index(blocks[b], new_file[b] != 0);
          tm.h2d_ms += ap.times.h2d_ms;
          tm.map_ms += ap.times.map_ms;
          tm.process_ms += ap.times.process_ms;
          tm.reduce_ms += ap.times.reduce_ms;
          tm.gpu_ms += ap.times.gpu_ms;
          index_ms += ap.index_ms;
          append_ms += ap.append_ms;
          if (a.keep_given && b + 1 - oldest > a.keep_blocks) {
            const IndexDrop dr = eng.drop_index(blocks[oldest++].num_lines);
            tm.gpu_ms += dr.drop_ms;
            drop_ms += dr.drop_ms;
            first_line = dr.first_line;
            g_dropped_files += dr.dropped_files;
          }
        }
        if (!a.queries.empty()) {
          sr = eng.search_resident(a.queries, a.rank, a.ignore_case, a.show, a.tally, a.by_file);
          tm.gpu_ms += sr.times.gpu_ms;
          sr.times = tm;
          sr.index_ms = index_ms;
          sr.times.wall_ms = (now_ns() - t0) * 1e-6;
          if (i >= a.warmup) walls.push_back(sr.times.wall_ms);
        } else {
          x = eng.index_resident();
          x.words.times = tm;
          x.index_ms = index_ms;
          x.words.times.wall_ms = (now_ns() - t0) * 1e-6;
          if (i >= a.warmup) walls.push_back(x.words.times.wall_ms);
        }
        g_blocks = blocks.size();
        g_append_ms = append_ms;
        g_store_bytes = eng.stats().index_store_bytes;
        g_dropped_blocks = oldest;
        g_drop_ms = drop_ms;
        g_first_line = first_line;
      }
      if (!a.queries.empty())
        print_gpu_result(a, search_stats(sr), walls, nullptr, nullptr, &sr);
      else
        print_gpu_result(a, x.words, walls, nullptr, &x);
      return 0;
    }
    GpuWordCount eng(a.cfg, text.input.bytes, text.input.num_lines);
    if (!a.queries.empty()) {  // the word job, the index stage and the search stage
      SearchResult sr;
      for (int i = 0; i < a.warmup + a.iters; ++i) {
        sr = eng.run_search(text.input, a.queries, a.rank, a.ignore_case, a.show, a.tally,
                            a.by_file);
        if (i >= a.warmup) walls.push_back(sr.times.wall_ms);
      }
      print_gpu_result(a, search_stats(sr), walls, nullptr, nullptr, &sr);
      return 0;
    }
    if (a.index) {  // the word job, then the index stage behind it on the device
      IndexResult x;
      for (int i = 0; i < a.warmup + a.iters; ++i) {
        x = eng.run_index(text.input);
        if (i >= a.warmup) walls.push_back(x.words.times.wall_ms);
      }
      print_gpu_result(a, x.words, walls, nullptr, &x);
      return 0;
    }
    if (a.top) {  // the selection runs on the device: only the winners come back
      TopResult top;
      for (int i = 0; i < a.warmup + a.iters; ++i) {
        top = eng.run_top(text.input, (u32)std::min<u64>(a.top, 0xFFFFFFFFu));
        if (i >= a.warmup) walls.push_back(top.times.wall_ms);
      }
      print_gpu_result(a, top_stats(top), walls, &top);
      return 0;
    }
    for (int i = 0; i < a.warmup; ++i) eng.run(text.input);
    for (int i = 0; i < a.iters; ++i) {
      r = eng.run(text.input);
      walls.push_back(r.times.wall_ms);
    }
    print_gpu_result(a, r, walls);
    return 0;
  }
  if (r.truncated)
    LOCUST_LOG_WARN("%llu tokens longer than %d chars were truncated",
                    (unsigned long long)r.truncated, a.cfg.max_key_len);
  std::string out;
  if (!a.queries.empty()) {
    if (!a.quiet) format_search_by_file(a, cpu_search, &out);
    g_search = &cpu_search;
  } else if (a.index) {
    if (!a.quiet) format_index_output(cpu_index, &out);
    g_index = &cpu_index;
  } else if (a.top) {
    format_top(a, cpu, cpu_top, &out);
  } else {
    format_results(a, cpu, r, &out);
  }
  emit_results(a, out);
  write_json(a, r, walls);
  if (!a.export_kiv.empty()) write_kiv_results(a.export_kiv, r);
  std::printf("\nDone\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  // before any thread or RCCL use (see locust_amd/__init__.py); a user's setting wins
  g_startup.main = now_ns();
  setenv("NCCL_GRAPH_REGISTER", "0", 0);
  for (int i = 1; i < argc; ++i)
    if (std::strcmp(argv[i], "--help") == 0 || std::strcmp(argv[i], "-h") == 0) {
      help();
      return 0;
    }
  std::printf("Running\n");
  CliArgs a;
  try {
    if (!parse(argc, argv, &a)) {
      usage();
      return -1;
    }
    const int rc = run(a);
    if (rc == 0 && (g_fast_exit || (a.cfg.backend == Backend::kGpu && fast_exit_ok()))) {
      std::fflush(nullptr);
      _exit(0);  // skip the HIP runtime's teardown (fast_exit_ok)
    }
    return rc;
  } catch (const std::exception& e) {
    std::fflush(stdout);
    std::fprintf(stderr, "MapReduce: error: %s\n", e.what());
    return 2;
  }
}
