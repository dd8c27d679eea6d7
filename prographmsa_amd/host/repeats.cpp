// repeats.cpp — tandem repeats (-R --read_repeats): the parser of the T-REKS report, the annotation of a leaf with its repeats and
// the repeat units of a child carried into a merged graph (reference src/RepeatDetectionTReks.cpp, ProgressiveAlignment.{h,cpp}).
#include "progressive_internal.h"

#include <algorithm>
#include <fstream>
#include <iostream>
#include <sstream>

namespace pgm {

// extend_tr_homologies (ProgressiveAlignment.h:266-287)
void extend_tr_homologies(ProgressiveAlignmentResult &result, const std::vector<index_t> &mapping, const std::vector<std::vector<int>> &tr_homologies,
                          const std::vector<std::string> &tr_source) {
    const index_t n = result.graph.size();
    for (size_t r = 0; r < tr_homologies.size(); ++r) {
        std::vector<int> extended(n - 2, -1);
        const std::vector<int> &original = tr_homologies[r];
        index_t k = 0;
        for (index_t j = 1; j < n - 1; ++j) extended[j - 1] = mapping[j] != (index_t)-1 ? original[k++] : -1;
        result.tr_homologies.push_back(extended);
        result.tr_source.push_back(tr_source[r]);
    }
}

// --read_repeats: the T-REKS report (RepeatDetectionTReks.cpp:62-151).  Per sequence ('>' line) any number of repeats: a header
// line "Length: ... from S to E ..." (S 1-based), then the aligned repeat units, one per line, up to a line of asterisks; '-',
// blanks and tabs are gaps; the residues of the units must spell the sequence from position S on.
static std::string strip_ws(const std::string &s) {
    size_t b = 0, e = s.size();
    while (b < e && isspace((unsigned char)s[b])) ++b;
    while (e > b && isspace((unsigned char)s[e - 1])) --e;
    return s.substr(b, e - b);
}
std::map<std::string, std::vector<repeat_t>> read_repeats(const Alphabet &a, const std::string &filename, const std::map<std::string, sequence_t> &seqs) {
    std::map<std::string, std::string> seqs2;
    for (const auto &kv : seqs) seqs2[kv.first] = stringFromSequence(a, kv.second);
    std::ifstream in(filename.c_str());
    std::map<std::string, std::vector<repeat_t>> map;
    index_t n_sequences = 0, n_repeats = 0;
    std::string name, line;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') { name = strip_ws(line.substr(1)); ++n_sequences; }
        else if (line.compare(0, 7, "Length:") == 0) {
            const size_t from = line.find("from");
            if (from == line.npos) throw pgm_exception("format error (from)");
            const size_t to = line.find("to", from);
            if (to == line.npos) throw pgm_exception("format error (to)");
            repeat_t repeat;
            ++n_repeats;
            long start = 0;
            { std::stringstream ss; ss << line.substr(from + 4, to - from - 4); ss >> start; if (!ss || start <= 0) throw pgm_exception("format error (number)"); }
            repeat.start = (index_t)(start - 1);
            auto orig_entry = seqs2.find(name);
            if (orig_entry == seqs2.end()) throw pgm_exception("unknown sequence name: " + name);
            size_t orig = repeat.start;
            repeat.len = (index_t)-1;
            while (std::getline(in, line)) {
                line = strip_ws(line);
                if (line.compare(0, 22, "**********************") == 0) break;
                for (char &c : line) if (c == '-' || c == ' ' || c == '\n' || c == '\t' || c == '\r') c = '_';
                if (repeat.len != (index_t)-1 && line.size() != repeat.len) throw pgm_exception("repeat unit lengths differ");
                repeat.len = (index_t)line.size();
                for (index_t i = 0; i < repeat.len; ++i)
                    if (line[i] != '_') {
                        repeat.tr_hom.push_back((int)i);
                        if (orig >= orig_entry->second.size() || orig_entry->second[orig] != line[i]) throw pgm_exception("character mismatch in repeat of \"" + name + "\"");
                        ++orig;
                    }
            }
            map[name].push_back(repeat);
        }
    }
    std::cerr << "found " << n_repeats << " repeats in " << n_sequences << " sequences" << std::endl;
    return map;
}

// tandem-repeat annotation of the leaves (ProgressiveAlignment.cpp:30-38)
void attach_repeats(ProgressiveAlignmentResult &res, const std::string &name, const std::map<std::string, std::vector<repeat_t>> &repeats) {
    auto it2 = repeats.find(name);
    if (it2 == repeats.end()) return;
    for (const repeat_t &rep : it2->second) {
        std::vector<int> tr_hom(res.graph.size(), -1);
        if ((size_t)rep.start + 1 + rep.tr_hom.size() > tr_hom.size()) error("repeat beyond the end of sequence %s", name.c_str());
        std::copy(rep.tr_hom.begin(), rep.tr_hom.end(), tr_hom.begin() + rep.start + 1);
        res.tr_homologies.push_back(tr_hom);
        res.tr_source.push_back(name);
    }
    res.graph.addRepeats(res.tr_homologies);
}

}  // namespace pgm
