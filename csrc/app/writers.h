// Native detection-product writers: ${prefix}${counter}.bin / .N.npy /
// .L.tim (formats identical to the reference write_signal_pipe.hpp:150-280
// and the unit-tested Python twin srtb_amd/io/writers.py).
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <sys/stat.h>
#include <vector>

namespace srtb_app {

inline bool file_exists(const std::string& p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0;
}

inline void write_baseband_bin(const std::string& prefix, uint64_t counter,
                               const uint8_t* data, size_t bytes) {
  const std::string path = prefix + std::to_string(counter) + ".bin";
  const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) throw std::runtime_error("cannot open " + path);
  size_t off = 0;
  while (off < bytes) {
    const ssize_t w = ::write(fd, data + off, bytes - off);
    if (w <= 0) break;
    off += (size_t)w;
  }
  ::fdatasync(fd);  // reference fdatasyncs baseband dumps
  ::close(fd);
}

// minimal .npy (format 1.0) writer for complex64 [rows][cols]; the
// per-polarization index is claimed with O_EXCL so concurrent pool writers
// (both pols of one block) get distinct .i.npy names
inline void write_spectrum_npy(const std::string& prefix, uint64_t counter,
                               const std::complex<float>* data, size_t rows,
                               size_t cols) {
  int fd = -1;
  for (int i = 0;; ++i) {  // multiple polarizations: first free index
    const std::string path = prefix + std::to_string(counter) + "." +
                             std::to_string(i) + ".npy";
    fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
    if (fd >= 0) break;
    if (errno != EEXIST)
      throw std::runtime_error("cannot create " + path);
  }
  std::ostringstream hd;
  hd << "{'descr': '<c8', 'fortran_order': False, 'shape': (" << rows << ", "
     << cols << "), }";
  std::string header = hd.str();
  const size_t total = 10 + header.size() + 1;
  const size_t pad = (64 - total % 64) % 64;
  header += std::string(pad, ' ');
  header += '\n';
  std::string head;
  head += std::string("\x93NUMPY\x01", 8 - 1);
  head += '\0';
  const uint16_t hlen = (uint16_t)header.size();
  head.append(reinterpret_cast<const char*>(&hlen), 2);
  head += header;
  size_t off = 0;
  while (off < head.size()) {
    const ssize_t w = ::write(fd, head.data() + off, head.size() - off);
    if (w <= 0) break;
    off += (size_t)w;
  }
  const char* body = reinterpret_cast<const char*>(data);
  const size_t nbytes = rows * cols * sizeof(std::complex<float>);
  off = 0;
  while (off < nbytes) {
    const ssize_t w = ::write(fd, body + off, nbytes - off);
    if (w <= 0) break;
    off += (size_t)w;
  }
  ::close(fd);
}

// sigproc filterbank header, byte-identical to the Python twin
// srtb_amd.io.writers.filterbank_header with its default telescope_id,
// machine_id, data_type, source_name and coordinates.
struct FilterbankHeader {
  double fch1 = 0, foff = 0, tsamp = 0, tstart = 0;
  int nchans = 0, nbits = 32;
  int nifs = 1;  // > 1: the data is [rows][nifs][nchans]
};

inline std::string filterbank_header(const FilterbankHeader& h) {
  std::string out;
  auto put_str = [&](const std::string& s) {
    const int32_t n = (int32_t)s.size();
    out.append(reinterpret_cast<const char*>(&n), 4);
    out += s;
  };
  auto put_int = [&](const char* key, int32_t v) {
    put_str(key);
    out.append(reinterpret_cast<const char*>(&v), 4);
  };
  auto put_real = [&](const char* key, double v) {
    put_str(key);
    out.append(reinterpret_cast<const char*>(&v), 8);
  };
  put_str("HEADER_START");
  put_int("telescope_id", 0);
  put_int("machine_id", 0);
  put_int("data_type", 1);
  put_real("fch1", h.fch1);
  put_real("foff", h.foff);
  put_int("nchans", h.nchans);
  put_real("tsamp", h.tsamp);
  put_real("tstart", h.tstart);
  put_int("nbits", h.nbits);
  put_int("nifs", h.nifs);
  put_real("src_raj", 0.0);
  put_real("src_dej", 0.0);
  put_str("source_name");
  put_str("srtb");
  put_str("HEADER_END");
  return out;
}

// `name.ext` -> `name<tag>.ext` (the tag goes before the extension)
inline std::string tag_before_extension(const std::string& path,
                                        const std::string& tag) {
  const size_t slash = path.rfind('/');
  size_t dot = path.rfind('.');
  if (dot == std::string::npos ||
      (slash != std::string::npos && dot < slash))
    dot = path.size();
  return path.substr(0, dot) + tag + path.substr(dot);
}

// .npy (format 1.0) of a C-ordered array: descr "<f8" or "<u8", shape
// "(rows, cols)" or "(n,)"
inline void write_npy_file(const std::string& path, const char* descr,
                           const std::string& shape, const void* data,
                           size_t nbytes) {
  std::string header = std::string("{'descr': '") + descr +
                       "', 'fortran_order': False, 'shape': " + shape + ", }";
  const size_t total = 10 + header.size() + 1;
  header += std::string((64 - total % 64) % 64, ' ');
  header += '\n';
  std::string head("\x93NUMPY\x01", 7);
  head += '\0';
  const uint16_t hlen = (uint16_t)header.size();
  head.append(reinterpret_cast<const char*>(&hlen), 2);
  head += header;
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  if (!f) throw std::runtime_error("cannot open " + path);
  f.write(head.data(), (std::streamsize)head.size());
  f.write(static_cast<const char*>(data), (std::streamsize)nbytes);
}

// One folded sub-integration, twin of the Python write_fold_subint:
// {stem}_{index:04d}.npy (float64 [S][nbin], waterfall row order),
// .hits.npy (uint64 [nbin]), .weights.npy (uint64 [S]) and .txt, whose
// `key = value` lines the caller supplies.
inline void write_fold_subint(const std::string& stem, unsigned index,
                              const std::vector<double>& acc,
                              const std::vector<uint64_t>& hits,
                              const std::vector<uint64_t>& weights,
                              const std::string& meta) {
  char num[16];
  std::snprintf(num, sizeof num, "_%04u", index);
  const std::string base = stem + num;
  const size_t S = weights.size(), nbin = hits.size();
  write_npy_file(base + ".npy", "<f8",
                 "(" + std::to_string(S) + ", " + std::to_string(nbin) + ")",
                 acc.data(), acc.size() * sizeof(double));
  write_npy_file(base + ".hits.npy", "<u8", "(" + std::to_string(nbin) + ",)",
                 hits.data(), hits.size() * sizeof(uint64_t));
  write_npy_file(base + ".weights.npy", "<u8", "(" + std::to_string(S) + ",)",
                 weights.data(), weights.size() * sizeof(uint64_t));
  std::ofstream f(base + ".txt", std::ios::trunc);
  f << meta;
}

inline void write_time_series_tim(const std::string& prefix, uint64_t counter,
                                  size_t boxcar, const float* data,
                                  size_t n) {
  const std::string path = prefix + std::to_string(counter) + "." +
                           std::to_string(boxcar) + ".tim";
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(data), n * sizeof(float));
}

}  // namespace srtb_app
