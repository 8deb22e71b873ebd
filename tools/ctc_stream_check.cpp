// CPU driver of the decode-stream arithmetic in tfkaldi_amd/csrc/ctc_tables.h for tests/test_ctc_stream_host.py: the limits of a
// stream's shape, the checks of a push and of a result, and the layout of its one allocation, called as the library calls them
// (ctc_entries.hip).  One command per line on stdin, fields separated by ';', arrays as blank-separated integers ("NULL" is a
// null pointer); one line per command on stdout.
//   limits;O;lanes;W;max_frames;label_topk          -> rc;message
//   push;T;max_frames;chunk_len...;frames...        -> rc;message
//   result;W;top_paths;hyp_cap                      -> rc;message
//   layout;lanes;W;max_frames                       -> trie hdr arr seg bytes lane_trie_words
// The numbers of the search are ctc.h's (kCtcBeamMaxWidth, kCtcBeamMaxClasses, kCtcBeamMaxFrames, kCtcTopkMaxClasses,
// kCtcTopkMaxLabels, kCtcStreamHdrWords, kCtcStreamArrays), which needs HIP and so is not included here.
#include "ctc_tables.h"

#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static std::string g_msg;
namespace tfk {
int set_error(int code, const char* msg) {
  g_msg = msg;
  return code;
}
}  // namespace tfk

namespace {

constexpr tfk::CtcStreamCaps kCaps = {128, 64, (1 << 19) - 2, 65536, 63, tfk::kCtcStreamMaxLanes};
constexpr int kHdrWords = 8, kArrays = 11;

std::vector<std::string> split(const std::string& line) {
  std::vector<std::string> out;
  std::string field;
  std::istringstream in(line);
  while (std::getline(in, field, ';')) out.push_back(field);
  if (!line.empty() && line.back() == ';') out.push_back("");
  return out;
}

std::vector<int32_t> array(const std::string& field, bool* null = nullptr) {
  std::vector<int32_t> out;
  if (null) *null = field == "NULL";
  if (field == "NULL") return out;
  std::istringstream in(field);
  long v;
  while (in >> v) out.push_back((int32_t)v);
  return out;
}

int num(const std::string& s) { return atoi(s.c_str()); }

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    const std::vector<std::string> f = split(line);
    const std::string& cmd = f[0];
    g_msg.clear();
    if (cmd == "limits" && f.size() == 6) {
      const int rc = tfk::ctc_stream_limits("stream", kCaps, num(f[1]), num(f[2]), num(f[3]), num(f[4]), num(f[5]));
      std::cout << rc << ";" << g_msg << "\n";
    } else if (cmd == "push" && f.size() == 5) {
      bool null = false;
      const std::vector<int32_t> chunk = array(f[3], &null), frames = array(f[4]);
      const int rc = tfk::ctc_stream_push_check("push", null ? nullptr : chunk.data(), frames.data(), (int)frames.size(),
                                                num(f[1]), num(f[2]));
      std::cout << rc << ";" << g_msg << "\n";
    } else if (cmd == "result" && f.size() == 4) {
      const int rc = tfk::ctc_stream_result_check("result", num(f[1]), num(f[2]), num(f[3]));
      std::cout << rc << ";" << g_msg << "\n";
    } else if (cmd == "layout" && f.size() == 4) {
      const tfk::CtcStreamLayout L = tfk::ctc_stream_layout(num(f[1]), num(f[2]), num(f[3]), kHdrWords, kArrays);
      std::cout << L.trie << " " << L.hdr << " " << L.arr << " " << L.seg << " " << L.bytes << " " << L.lane_trie_words << "\n";
    } else {
      std::cerr << "bad command: " << line << "\n";
      return 2;
    }
  }
  return 0;
}
