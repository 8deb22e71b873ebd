// CPU driver of tfkaldi_amd/csrc/ctc_tables.h for tests/test_ctc_tables_host.py: the checks the CTC entries run on their small
// tables, and the layout of a CtcBatch in one allocation, called as the library calls them.  One command per line on stdin,
// fields separated by ';', arrays as blank-separated integers ("512*0" repeats a value, "NULL" is a null pointer, "-" an
// empty array); one line per command on stdout: the return code, the message (empty on success) and the outputs.
//   seg;family;whole;T;seg...                                   -> rc;message
//   off;family;unit;noun;limit;off...                           -> rc;message;longest
//   pairs;family;U;ordered;pair_utt...;off...                   -> rc;message;longest
//   trans;family;O;limit;T;utt_len...;label_len...;labels;wild  -> rc;message;total
//   count;family;noun;max_pairs;hyp_count...;utt_len...         -> rc;message;P
//   build;family;noun;name_pair;O;limit;hyp_count...;label_len...;labels;wild -> rc;message;longest;total;pair_utt...;lab_off...
//   layout;T;U;ld;sext;lead;mid;tail                            -> the twelve fields of CtcBatchLayout
#include "ctc_tables.h"

#include <stdlib.h>
#include <string.h>

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

std::vector<std::string> split(const std::string& line) {
  std::vector<std::string> out;
  std::string field;
  std::istringstream in(line);
  while (std::getline(in, field, ';')) out.push_back(field);
  if (!line.empty() && line.back() == ';') out.push_back("");
  return out;
}

// an array field; *null is set for "NULL"
template <class Tp>
std::vector<Tp> array(const std::string& field, bool* null = nullptr) {
  std::vector<Tp> out;
  if (null) *null = field == "NULL";
  if (field == "NULL" || field == "-") return out;
  std::istringstream in(field);
  std::string item;
  while (in >> item) {
    const size_t star = item.find('*');
    const long count = star == std::string::npos ? 1 : atol(item.substr(0, star).c_str());
    const long value = atol(star == std::string::npos ? item.c_str() : item.c_str() + star + 1);
    out.insert(out.end(), (size_t)count, (Tp)value);
  }
  return out;
}

std::string join(const std::vector<int32_t>& v) {
  std::ostringstream out;
  for (size_t i = 0; i < v.size(); ++i) out << (i ? " " : "") << v[i];
  return out.str();
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    const std::vector<std::string> f = split(line);
    const std::string& cmd = f[0];
    g_msg.clear();
    if (cmd == "seg" && f.size() == 5) {
      const std::vector<int32_t> seg = array<int32_t>(f[4]);
      const int rc = tfk::seg_check(f[1].c_str(), seg.data(), (int)seg.size() - 1, atoi(f[3].c_str()), atoi(f[2].c_str()) != 0);
      std::cout << rc << ";" << g_msg << "\n";
    } else if (cmd == "off" && f.size() == 6) {
      const std::vector<int32_t> off = array<int32_t>(f[5]);
      int longest = -1;
      const int rc = tfk::offsets_check(f[1].c_str(), f[2].c_str(), f[3].c_str(), off.data(), (int)off.size() - 1,
                                        atoi(f[4].c_str()), &longest);
      std::cout << rc << ";" << g_msg << ";" << longest << "\n";
    } else if (cmd == "pairs" && f.size() == 6) {
      const std::vector<int32_t> utt = array<int32_t>(f[4]), off = array<int32_t>(f[5]);
      int longest = -1;
      const int rc = tfk::pairs_check(f[1].c_str(), utt.data(), off.data(), (int)utt.size(), atoi(f[2].c_str()),
                                      atoi(f[3].c_str()) != 0, &longest);
      std::cout << rc << ";" << g_msg << ";" << longest << "\n";
    } else if (cmd == "trans" && f.size() == 9) {
      bool no_labels = false, no_wild = false;
      const std::vector<int32_t> utt = array<int32_t>(f[5]), len = array<int32_t>(f[6]), labels = array<int32_t>(f[7], &no_labels);
      const std::vector<uint8_t> wild = array<uint8_t>(f[8], &no_wild);
      int64_t total = -1;
      const int rc = tfk::transcripts_check(f[1].c_str(), utt.data(), len.data(), no_labels ? nullptr : labels.data(),
                                            no_wild ? nullptr : wild.data(), (int)utt.size(), atoi(f[2].c_str()),
                                            atoi(f[3].c_str()), atoi(f[4].c_str()), &total);
      std::cout << rc << ";" << g_msg << ";" << total << "\n";
    } else if (cmd == "count" && f.size() == 6) {
      const std::vector<int32_t> count = array<int32_t>(f[4]), utt = array<int32_t>(f[5]);
      int P = -1;
      const int rc = tfk::pairs_count(f[1].c_str(), f[2].c_str(), count.data(), utt.data(), (int)count.size(), atoi(f[3].c_str()), &P);
      std::cout << rc << ";" << g_msg << ";" << P << "\n";
    } else if (cmd == "build" && f.size() == 10) {
      bool no_labels = false, no_wild = false;
      const std::vector<int32_t> count = array<int32_t>(f[6]), len = array<int32_t>(f[7]), labels = array<int32_t>(f[8], &no_labels);
      const std::vector<uint8_t> wild = array<uint8_t>(f[9], &no_wild);
      std::vector<int32_t> pair_utt(len.size(), -1), lab_off(len.size() + 1, -1);
      int longest = -1;
      int64_t total = -1;
      const int rc = tfk::pairs_build(f[1].c_str(), f[2].c_str(), atoi(f[3].c_str()) != 0, count.data(), (int)count.size(),
                                      len.data(), no_labels ? nullptr : labels.data(), no_wild ? nullptr : wild.data(),
                                      atoi(f[4].c_str()), atoi(f[5].c_str()), pair_utt.data(), lab_off.data(), &longest, &total);
      std::cout << rc << ";" << g_msg << ";" << longest << ";" << total << ";" << join(pair_utt) << ";" << join(lab_off) << "\n";
    } else if (cmd == "layout" && f.size() == 8) {
      const tfk::CtcBatchLayout L =
          tfk::ctc_batch_layout(atoi(f[1].c_str()), atoi(f[2].c_str()), atoll(f[3].c_str()), atoi(f[4].c_str()),
                                (size_t)atoll(f[5].c_str()), (size_t)atoll(f[6].c_str()), (size_t)atoll(f[7].c_str()));
      std::cout << L.lead << " " << L.off << " " << L.offb << " " << L.logz << " " << L.post << " " << L.mid << " " << L.lp << " "
                << L.ab << " " << L.bb << " " << L.lse << " " << L.tail << " " << L.bytes << "\n";
    } else {
      std::cerr << "bad command: " << line << "\n";
      return 2;
    }
  }
  return 0;
}
