// bscanfft_sim.cpp -- headless counterpart of the reference's simulation harness
// (BscanFFTsim.cpp: "simulation using saved files, for testing and validation").
//
// The reference's loop (sim:775-1131) reads imgi.png each iteration, runs the OpenCV processing block
// (sim:842-955) and shows the B-scan; 'b' loads backg.png as data_yb (sim:803-813).  This program does the
// same through the C ABI of include/fdoct.h on an MI355X, from raw frame files (no OpenCV, no GUI):
//
//   bscanfft_sim --frames imgi_u16_96x128.bin --background backg_u16_96x128.bin
//                --width 128 --height 96 --bits 16 --numfftpoints 1024 --numdisplaypoints 512
//                [--averages A] [--sim] [--lambdamin 816e-9 --lambdamax 884e-9]
//                [--rowwisenormalize 0|1] [--donotnormalize 0|1] [--repeat K] [--threshold dB] --out prefix
//                [--gpus N [--devices d0,d1,...]] [--precise-division | --one-word-division]
//                [--roi-mean ascanat,vertpos,width] [--capture-background N [--capture-lowpass] [--capture-raw]] [--max-intensity]
//                [--calibrate-dark-ref-sample N [--capture-lowpass] [--capture-raw]]
//                [--bscan-bin BX,BY[,BINVALUEX,BINVALUEY]] [--channel N] [--manual-averages M [--manual-keep-all]] [--save-frames]
//
// --gpus N: one process, N handles (fdoct_clone_to_device), one host thread per handle; the frames are sharded with
// fdoct_shard_frames (contiguous ranges, averaging groups never split -- the rule of the multi-process path,
// fdoct_amd/dist.py) and every handle writes its B-scans straight into its slice of the output.  No collective: the only
// exchange is the clone of the constant state.  --devices lists the device of each handle (default 0, 1, ..., wrapping
// around when fewer GPUs are visible -- several handles then share a device, which is how a 1-GPU box rehearses it).
//
// --roi-mean: the ROIreport readout of printAvgROI (BscanFFT.cpp:99-144) on every output B-scan, one line per B-scan in
// the reference's text ("Mean of ROI at <ascanat> = <mean> dB"), computed on the GPU (include/fdoct_roi.h).
// --capture-background N: the 'b' key of the acquisition programs (BscanFFT.cpp:1000-1075) instead of a background file: the
// first N frames of --frames are accumulated and normalised into data_yb on the GPU (include/fdoct_capture.h) and are not
// reconstructed; --background is then not needed.  --capture-lowpass ends that capture with BscanDark's lpfilter (the ini's
// lowpassfilter), --capture-raw skips its moving average (the ini's saveinterferograms; include/fdoct_lowpass.h); with either,
// the captured frame is also written as <prefix>_background.f64 (H x W doubles).
// --calibrate-dark-ref-sample N: BscanDark's calibration (BscanDark.cpp:996, 1005-1222) instead of a background file: the first
// 3 N frames of --frames are the dark, the reference-arm and the sample-arm capture of N frames each (the d / r / t keys), made
// and held on the GPU (include/fdoct_calibrate.h); the dark capture becomes data_yd, and data_yb = (yr - yd) + (ys - yd) is
// composed there from the three.  Those frames are not reconstructed, --background is not needed, and the composed frame is
// written as <prefix>_background.f64.  --capture-lowpass and --capture-raw act on the three captures as they do on the 'b' key's.
// --bscan-bin BX,BY[,BINVALUEX,BINVALUEY]: spinjnt's output binning (bscanbinx, bscanbiny and the software binvalues;
// BscanFFTspinjnt.cpp:1856-1861) on every output B-scan between the chain and everything written below, on the GPU
// (include/fdoct_bscanbin.h), with the reference's own arguments: upx = BX * BINVALUEY, upy = BY and multiplyfactor =
// BX * BY * BINVALUEX * BINVALUEY (835).  The outputs then have (D / BY) * upy depths and (H / BX) * upx A-scans.
// --channel N: BscanFFTwebcam.ini's channelnum (BscanFFTwebcam.cpp:1015-1038).  --frames then holds 8-bit, 3-channel
// interleaved B,G,R frames -- a 3-channel .ocv dump, or raw H x W x 3 bytes -- and the GPU takes channel N (0, 1, 2 = B, G, R) or
// the scaled sum (3) of every frame (include/fdoct_colour.h) ahead of the capture, the chain and the max-intensity line.  A
// --background file stays a mono frame or spectrum of --bits samples.
// --manual-averages M: the ini's manualaveraging with manualaverages = M (BscanFFT.cpp:1399-1444) over the output B-scans, in order,
// on the GPU (include/fdoct_manualavg.h): every M + 1 B-scans give one averaged image -- the B-scan that arrives when M are in is
// dropped, as in the reference; with --manual-keep-all every M give one and nothing is dropped.  The emitted images are written
// as <prefix>_bscanman.f32 (manualaccum / M, what 1440 saves before its log) and <prefix>_bscanman_db.f32 (20 ln / 2.303), D x H
// each; B-scans left in the accumulator at the end are reported and not written.
// --save-frames: the ini's save_individual_frames_if_averaging (BscanFFT.cpp:1198-1205, 1360-1377; include/fdoct_saveframes.h).
// The chain then runs once per camera frame -- averages = 1 with raw magnitudes on, so it writes every frame's own magnitudes --
// and fdoct_saveframes makes from them the averaged B-scans (sums in double, as the reference accumulates) and every frame's
// save picture, written as <prefix>_bscanNNN-III.pgm (D x H; NNN the B-scan from 001, III the frame of its group from 000, as
// the reference counts them).  The reference saves the PREVIOUS group's frames on `s`; this writes every group's own.
// --max-intensity: the status line's "Max intensity = <floor(max)>" (BscanFFT.cpp:1105-1108) for every reconstructed frame.
// --frames holds one or more H x W frames back to back (u8 for --bits 8, little-endian u16 for --bits 16).
// Outputs: <prefix>_bscan.f32 / <prefix>_bscandb.f32 (reference layout D x H per B-scan, main:1220) and
// <prefix>.m with `bscan001=[...];` in the Matlab text form the reference's savematasdata writes
// (main:333-339) for the first B-scan, plus the display images the reference shows/saves (main:1242-1255, 1284,
// savematasimage): <prefix>_bscan001.pgm (grey) and <prefix>_bscanc001.ppm (colour-mapped).  Prints A-scans/s like the reference prints fps (sim:827-838).
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "../include/fdoct.h"
#include "../include/fdoct_bscanbin.h"
#include "../include/fdoct_calibrate.h"
#include "../include/fdoct_capture.h"
#include "../include/fdoct_colour.h"
#include "../include/fdoct_lowpass.h"
#include "../include/fdoct_manualavg.h"
#include "../include/fdoct_roi.h"
#include "../include/fdoct_saveframes.h"
#include "ocv_io.h"

static bool ends_with(const std::string& s, const std::string& suf) {
  return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

static std::vector<unsigned char> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(1);
  }
  return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  std::string frames_path, bg_path, out = "bscanfft_sim";
  fdoct_config cfg;
  std::memset(&cfg, 0, sizeof cfg);
  cfg.struct_size = sizeof cfg;
  cfg.increasefftpointsmultiplier = 1;
  cfg.averages = 1;
  cfg.donotnormalize = 1;  // build/BscanFFT.ini default
  cfg.dc_mask = 1;
  cfg.lambdamin = 816e-9;  // sim:276-277
  cfg.lambdamax = 884e-9;
  int bits = 16, repeat = 1, gpus = 1;
  int precise = -1;  // -1: the library default (both words of 1/background since round 5)
  std::vector<int> devices;
  double bscanthreshold = -30.0;  // main:385
  int roi[3] = {-1, 0, 0};         // --roi-mean ascanat,vertpos,width (-1: off)
  int capture_bg = 0;              // --capture-background N (0: read --background)
  int capture_lowpass = 0, capture_raw = 0;  // --capture-lowpass, --capture-raw: fdoct_set_capture_options
  int calibrate_n = 0;             // --calibrate-dark-ref-sample N (0: no calibration)
  bool max_intensity = false;      // --max-intensity
  int bbin[4] = {0, 0, 1, 1};      // --bscan-bin bscanbinx,bscanbiny[,binvaluex,binvaluey] (0: off)
  int channel = -1;                // --channel channelnum (-1: mono frames)
  int manual_averages = -1;        // --manual-averages manualaverages (-1: manualaveraging off)
  int manual_mode = FDOCT_MANUALAVG_REFERENCE;  // --manual-keep-all
  bool save_frames = false;        // --save-frames
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "missing value after %s\n", a.c_str());
        std::exit(1);
      }
      return argv[++i];
    };
    if (a == "--frames") frames_path = next();
    else if (a == "--background") bg_path = next();
    else if (a == "--out") out = next();
    else if (a == "--width") cfg.width = std::atoi(next());
    else if (a == "--height") cfg.height = std::atoi(next());
    else if (a == "--bits") bits = std::atoi(next());
    else if (a == "--numfftpoints") cfg.numfftpoints = std::atoi(next());
    else if (a == "--numdisplaypoints") cfg.numdisplaypoints = std::atoi(next());
    else if (a == "--averages") cfg.averages = std::atoi(next());
    else if (a == "--rowwisenormalize") cfg.rowwisenormalize = std::atoi(next());
    else if (a == "--donotnormalize") cfg.donotnormalize = std::atoi(next());
    else if (a == "--lambdamin") cfg.lambdamin = std::atof(next());
    else if (a == "--lambdamax") cfg.lambdamax = std::atof(next());
    else if (a == "--repeat") repeat = std::atoi(next());
    else if (a == "--threshold") bscanthreshold = std::atof(next());
    else if (a == "--sim") cfg.variant = FDOCT_VARIANT_SIM;
    else if (a == "--gpus") gpus = std::atoi(next());
    else if (a == "--precise-division") precise = 1;   // main:1132 divides in double: both words of 1/background on the fast path too (the default)
    else if (a == "--one-word-division") precise = 0;  // the opt-out: one f32 reciprocal on the fast path, for fringes above ~1 % of the DC level
    else if (a == "--roi-mean") {
      if (std::sscanf(next(), "%d,%d,%d", &roi[0], &roi[1], &roi[2]) != 3) {
        std::fprintf(stderr, "--roi-mean wants ascanat,vertpos,width\n");
        return 1;
      }
    }
    else if (a == "--bscan-bin") {
      const int n = std::sscanf(next(), "%d,%d,%d,%d", &bbin[0], &bbin[1], &bbin[2], &bbin[3]);
      if ((n != 2 && n != 4) || bbin[0] < 1 || bbin[1] < 1 || bbin[2] < 1 || bbin[3] < 1) {
        std::fprintf(stderr, "--bscan-bin wants BX,BY or BX,BY,BINVALUEX,BINVALUEY\n");
        return 1;
      }
    }
    else if (a == "--capture-background") capture_bg = std::atoi(next());
    else if (a == "--calibrate-dark-ref-sample") calibrate_n = std::atoi(next());
    else if (a == "--capture-lowpass") capture_lowpass = 1;
    else if (a == "--capture-raw") capture_raw = 1;
    else if (a == "--max-intensity") max_intensity = true;
    else if (a == "--channel") channel = std::atoi(next());
    else if (a == "--manual-averages") {
      manual_averages = std::atoi(next());
      if (manual_averages < 1) {
        std::fprintf(stderr, "--manual-averages wants a count of at least 1\n");
        return 1;
      }
    }
    else if (a == "--manual-keep-all") manual_mode = FDOCT_MANUALAVG_KEEP_ALL;
    else if (a == "--save-frames") save_frames = true;
    else if (a == "--devices") {
      for (const char* p = next(); *p;) {
        devices.push_back(std::atoi(p));
        while (*p && *p != ',') p++;
        if (*p == ',') p++;
      }
    }
    else {
      std::fprintf(stderr, "unknown option %s\n", a.c_str());
      return 1;
    }
  }
  if (calibrate_n < 0 || (calibrate_n > 0 && capture_bg > 0)) {
    std::fprintf(stderr, "--calibrate-dark-ref-sample takes a positive frame count and replaces --capture-background\n");
    return 1;
  }
  const int captured_frames = capture_bg + 3 * calibrate_n;  // the frames at the head of --frames that make the background
  if (frames_path.empty() || (bg_path.empty() && captured_frames <= 0) || capture_bg < 0 || cfg.width <= 0 || cfg.height <= 0 || cfg.numfftpoints <= 0) {
    std::fprintf(stderr, "usage: see the header of host/bscanfft_sim.cpp\n");
    return 1;
  }
  if (cfg.numdisplaypoints <= 0) cfg.numdisplaypoints = cfg.numfftpoints / 2;
  const fdoct_dtype dt = bits == 8 ? FDOCT_U8 : FDOCT_U16;
  const size_t es = bits == 8 ? 1 : 2;
  if (channel >= 0 && bits != 8) {
    std::fprintf(stderr, "--channel takes 8-bit B,G,R frames: give --bits 8\n");
    return 1;
  }
  if (save_frames && cfg.variant == FDOCT_VARIANT_SIM) {
    std::fprintf(stderr, "--save-frames folds the frames of a group: the sim variant copies and does not accumulate\n");
    return 1;
  }
  // --save-frames: the chain's handle takes the frames one by one; `averages` is the fold's
  const int averages = cfg.averages;
  if (save_frames) cfg.averages = 1;
  const int frame_channels = channel >= 0 ? 3 : 1;
  const size_t frame_bytes = (size_t)cfg.width * cfg.height * es * frame_channels;

  // frames saved by the instrument programs as .ocv Mat dumps (BscanFFTspinj.cpp:672-738) carry their own
  // geometry; raw .bin files take it from the command line
  std::vector<unsigned char> frames, bg;
  auto load = [&](const std::string& path, std::vector<unsigned char>* out, int channels) {
    if (ends_with(path, ".ocv")) {
      OcvMat m;
      if (!ocv_read(path, &m) || (m.depth != 0 && m.depth != 2) || m.channels != channels || m.cols != cfg.width) {
        std::fprintf(stderr, "%s: not a %d-channel 8/16-bit .ocv frame of width %d\n", path.c_str(), channels, cfg.width);
        std::exit(1);
      }
      if ((m.depth == 0 ? 8 : 16) != bits) {
        std::fprintf(stderr, "%s holds %d-bit samples, --bits says %d\n", path.c_str(), m.depth == 0 ? 8 : 16, bits);
        std::exit(1);
      }
      *out = m.data;
    } else {
      *out = read_file(path);
    }
  };
  load(frames_path, &frames, frame_channels);
  if (captured_frames == 0) load(bg_path, &bg, 1);
  const int nframes_file = (int)(frames.size() / frame_bytes) - captured_frames;  // (the captured frames are not reconstructed)
  const unsigned char* live = frames.data() + (size_t)captured_frames * frame_bytes;
  if (nframes_file < 1) {
    if (captured_frames > 0)
      std::fprintf(stderr, "%s: no frames are left to reconstruct after the %d captured as the background\n", frames_path.c_str(), captured_frames);
    else
      std::fprintf(stderr, "%s holds no complete %dx%d frame\n", frames_path.c_str(), cfg.width, cfg.height);
    return 1;
  }
  const int nframes = nframes_file / averages * averages;
  if (nframes < 1) {
    std::fprintf(stderr, "need at least `averages` frames\n");
    return 1;
  }
  int bg_rows = 0;
  if (captured_frames > 0) bg_rows = cfg.height;
  else if (bg.size() >= (size_t)cfg.width * cfg.height * es) bg_rows = cfg.height;
  else if (bg.size() >= (size_t)cfg.width * es) bg_rows = 1;
  else {
    std::fprintf(stderr, "background file too small\n");
    return 1;
  }

  fdoct_handle h = nullptr;
  int rc = fdoct_create(&cfg, &h);  // replaces the one-time set-up sim:385-534, 765-773
  if (rc) {
    std::fprintf(stderr, "fdoct_create: %d %s\n", rc, fdoct_last_error(nullptr));
    return 1;
  }
  if (channel >= 0 && (rc = fdoct_set_colour_input(h, channel))) {  // webcam:1015-1038: every frame below is B,G,R
    std::fprintf(stderr, "fdoct_set_colour_input: %s\n", fdoct_last_error(h));
    return 1;
  }
  // the 'b' key: data_yb <- backg (sim:803-813)
  const char* bg_call = capture_bg > 0 ? "fdoct_capture_reference" : "fdoct_set_background";
  if (calibrate_n > 0) {  // ... or BscanDark's d / r / t keys and BscanDark.cpp:996, all on the device
    bg_call = "fdoct_calibrate_capture";
    if ((rc = fdoct_set_capture_options(h, capture_lowpass, capture_raw))) {
      std::fprintf(stderr, "fdoct_set_capture_options: %s\n", fdoct_last_error(h));
      return 1;
    }
    const int slots[3] = {FDOCT_CAL_DARK, FDOCT_CAL_REFERENCE, FDOCT_CAL_SAMPLE};
    for (int k = 0; k < 3 && !rc; k++)
      rc = fdoct_calibrate_capture(h, slots[k], frames.data() + (size_t)k * calibrate_n * frame_bytes, dt, FDOCT_MEM_HOST, calibrate_n, 0, nullptr);
    if (!rc) {
      bg_call = "fdoct_calibrate_compose";
      std::vector<double> composed((size_t)cfg.width * cfg.height);
      rc = fdoct_calibrate_compose(h, composed.data());
      if (!rc) {
        std::ofstream f(out + "_background.f64", std::ios::binary);
        f.write(reinterpret_cast<const char*>(composed.data()), (std::streamsize)(composed.size() * sizeof(double)));
      }
    }
  } else if (capture_bg > 0) {  // ... or the live 'b' key: accumulate(data_y, baccum) over the first frames, main:1041-1064
    const bool options = capture_lowpass || capture_raw;
    std::vector<double> captured(options ? (size_t)cfg.width * cfg.height : 0);
    if (options && (rc = fdoct_set_capture_options(h, capture_lowpass, capture_raw))) {
      std::fprintf(stderr, "fdoct_set_capture_options: %s\n", fdoct_last_error(h));
      return 1;
    }
    rc = fdoct_capture_reference(h, FDOCT_REF_BACKGROUND, frames.data(), dt, FDOCT_MEM_HOST, capture_bg, 0,
                                 options ? captured.data() : nullptr);
    if (!rc && options) {
      std::ofstream f(out + "_background.f64", std::ios::binary);
      f.write(reinterpret_cast<const char*>(captured.data()), (std::streamsize)(captured.size() * sizeof(double)));
    }
  } else
    rc = fdoct_set_background(h, bg.data(), dt, bg_rows, 0);
  if (rc) {
    std::fprintf(stderr, "%s: %s\n", bg_call, fdoct_last_error(h));
    return 1;
  }
  if (precise >= 0 && (rc = fdoct_set_precise_division(h, precise))) {
    std::fprintf(stderr, "fdoct_set_precise_division: %s\n", fdoct_last_error(h));
    return 1;
  }
  if (save_frames && (rc = fdoct_set_raw_magnitudes(h, 1))) {
    std::fprintf(stderr, "fdoct_set_raw_magnitudes: %s\n", fdoct_last_error(h));
    return 1;
  }
  // before the loop: tables, kernel family and any run-time compile, so that the first frame does not stall (an acquisition
  // program would do the same after its 'b' key)
  const int prepared = fdoct_prepare(h, dt, save_frames ? FDOCT_LAYOUT_ROWMAJOR_HxD : FDOCT_LAYOUT_TRANSPOSED_DxH);
  if (prepared < 0) {
    std::fprintf(stderr, "fdoct_prepare: %d %s\n", prepared, fdoct_last_error(h));
    return 1;
  }
  const int G = nframes / averages;
  const size_t out_elems = (size_t)G * cfg.numdisplaypoints * cfg.height;
  std::vector<float> bscan(out_elems), bscandb(out_elems);
  // --save-frames: every frame's magnitudes (H x D, as the chain writes them) and its picture (D x H)
  std::vector<float> framemag(save_frames ? (size_t)nframes * cfg.numdisplaypoints * cfg.height : 0);
  std::vector<unsigned char> framegray(framemag.size());
  // one handle per GPU: clones of the configured handle, each on its own device and host thread
  if (gpus < 1) gpus = 1;
  const int ndev = fdoct_device_count();
  std::vector<fdoct_handle> hs(gpus, nullptr);
  hs[0] = h;
  for (int g = 1; g < gpus; g++) {
    const int dev = g < (int)devices.size() ? devices[g] : (ndev > 0 ? g % ndev : 0);
    rc = fdoct_clone_to_device(h, dev, &hs[g]);
    if (rc) {
      std::fprintf(stderr, "fdoct_clone_to_device(%d): %d %s\n", dev, rc, fdoct_last_error(h));
      return 1;
    }
  }
  std::vector<int> rcs(gpus, 0);
  const size_t bscan_elems = (size_t)cfg.numdisplaypoints * cfg.height;
  auto run_shard = [&](int g) {
    int first = 0, count = 0;
    fdoct_shard_frames(nframes, averages, g, gpus, &first, &count);
    if (count == 0) return;
    const size_t o0 = (size_t)(first / averages) * bscan_elems;
    for (int k = 0; k < repeat && !rcs[g]; k++) {  // the while(1) loop, bounded; sim:842-955 per iteration
      if (!save_frames) {
        rcs[g] = fdoct_process(hs[g], live + (size_t)first * frame_bytes, dt, FDOCT_MEM_HOST, count, 0, bscan.data() + o0,
                               bscandb.data() + o0, FDOCT_MEM_HOST, FDOCT_LAYOUT_TRANSPOSED_DxH);
        continue;
      }
      float* mag = framemag.data() + (size_t)first * bscan_elems;
      rcs[g] = fdoct_process(hs[g], live + (size_t)first * frame_bytes, dt, FDOCT_MEM_HOST, count, 0, mag, nullptr, FDOCT_MEM_HOST,
                             FDOCT_LAYOUT_ROWMAJOR_HxD);
      if (!rcs[g])
        rcs[g] = fdoct_saveframes(hs[g], mag, FDOCT_MEM_HOST, FDOCT_LAYOUT_ROWMAJOR_HxD, count, cfg.numdisplaypoints, cfg.height,
                                  framegray.data() + (size_t)first * bscan_elems, averages, bscan.data() + o0, bscandb.data() + o0,
                                  FDOCT_LAYOUT_TRANSPOSED_DxH, FDOCT_MEM_HOST);
    }
  };
  const auto t0 = std::chrono::steady_clock::now();
  if (gpus == 1) {
    run_shard(0);
  } else {
    std::vector<std::thread> th;
    for (int g = 0; g < gpus; g++) th.emplace_back(run_shard, g);
    for (auto& t : th) t.join();
  }
  for (int g = 0; g < gpus; g++)
    if (rcs[g]) {
      std::fprintf(stderr, "%s (handle %d): %d %s\n", save_frames ? "fdoct_process / fdoct_saveframes" : "fdoct_process", g, rcs[g], fdoct_last_error(hs[g]));
      return 1;
    }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  fdoct_timing tm;
  fdoct_get_timing(h, &tm);
  static const char* const family[] = {"none", "fused", "fused, D x H written by the chain", "fused, two stages", "wave per row",
                                       "wave per row, compiled for this geometry at run time", "workgroup per row", "long rows"};
  const int fam = fdoct_last_kernel(h);
  std::printf("%s: %d frame(s) x %d on %d handle(s), %d B-scan(s) %dx%d; %.0f A-scans/s incl. PCIe (device %.3f ms per call, kernel %.3f ms; %s kernel%s%s)\n",
              fdoct_version(), nframes, repeat, gpus, G, cfg.numdisplaypoints, cfg.height,
              (double)nframes * cfg.height * repeat / sec, tm.last_process_ms, tm.last_kernel_ms,
              fam >= 0 && fam < 8 ? family[fam] : "?", *fdoct_jit_note(h) ? "; " : "", fdoct_jit_note(h));

  if (save_frames) {
    // main:1375-1376: one picture per frame, named after its B-scan and its place in the group
    for (int f = 0; f < nframes; f++) {
      char name[64];
      std::snprintf(name, sizeof name, "_bscan%03d-%03d.pgm", f / averages + 1, f % averages);
      std::ofstream pg(out + name, std::ios::binary);
      pg << "P5\n" << cfg.height << " " << cfg.numdisplaypoints << "\n255\n";
      pg.write(reinterpret_cast<const char*>(framegray.data() + (size_t)f * bscan_elems), (std::streamsize)bscan_elems);
    }
    std::printf("save frames: %d picture(s) of %d B-scan(s) written\n", nframes, G);
  }

  // spinjnt's output stage (BscanFFTspinjnt.cpp:1856-1874): the averaged linear B-scan is binned and resized back, and the dB
  // (with the DC mask) is taken of the result; everything below sees these images, as in the reference
  int OD = cfg.numdisplaypoints, OH = cfg.height;
  if (bbin[0] > 0) {
    const int upx = bbin[0] * bbin[3], upy = bbin[1];  // 1861: bscanbinx * binvaluey (the reference's own quirk), bscanbiny
    const double multiplyfactor = (double)bbin[0] * bbin[1] * bbin[2] * bbin[3];  // 835
    const int size_rc = rc = fdoct_bscanbin_size(cfg.numdisplaypoints, cfg.height, bbin[0], bbin[1], upx, upy, &OD, &OH);
    std::vector<float> lin, db;
    if (!rc) {
      lin.resize((size_t)G * OD * OH), db.resize(lin.size());
      rc = fdoct_bscan_bin(h, bscan.data(), nullptr, FDOCT_MEM_HOST, FDOCT_LAYOUT_TRANSPOSED_DxH, G, cfg.numdisplaypoints, cfg.height,
                           bbin[0], bbin[1], upx, upy, multiplyfactor, lin.data(), db.data(), FDOCT_MEM_HOST);
    }
    if (rc) {
      std::fprintf(stderr, "fdoct_bscan_bin: %d %s\n", rc, fdoct_last_error(size_rc ? nullptr : h));
      return 1;
    }
    bscan.swap(lin);
    bscandb.swap(db);
  }

  if (manual_averages > 0) {
    // manualaveraging (main:1399-1444) over the B-scans as the loop would hand them over, one call for all of them
    const size_t px = (size_t)OD * OH;
    int emitted = 0, left = 0;
    rc = fdoct_manualavg_plan(manual_averages, manual_mode, 0, G, &emitted, &left);
    std::vector<float> man((size_t)emitted * px), mandb(man.size());
    if (!rc) rc = fdoct_manualavg_begin(h, manual_averages, px, manual_mode);
    if (!rc)
      rc = fdoct_manualavg_add(h, bscan.data(), FDOCT_MEM_HOST, G, emitted ? man.data() : nullptr, emitted ? mandb.data() : nullptr,
                               FDOCT_MEM_HOST, emitted, nullptr);
    if (!rc) rc = fdoct_manualavg_end(h);
    if (rc) {
      std::fprintf(stderr, "fdoct_manualavg: %d %s\n", rc, fdoct_last_error(h));
      return 1;
    }
    std::ofstream f(out + "_bscanman.f32", std::ios::binary);
    f.write(reinterpret_cast<const char*>(man.data()), (std::streamsize)(man.size() * sizeof(float)));
    std::ofstream g(out + "_bscanman_db.f32", std::ios::binary);
    g.write(reinterpret_cast<const char*>(mandb.data()), (std::streamsize)(mandb.size() * sizeof(float)));
    std::printf("manual averaging of %d: %d image(s) written, %d B-scan(s) left in the accumulator\n", manual_averages, emitted, left);
  }

  {
    std::ofstream f(out + "_bscan.f32", std::ios::binary);
    f.write(reinterpret_cast<const char*>(bscan.data()), bscan.size() * sizeof(float));
    std::ofstream g(out + "_bscandb.f32", std::ios::binary);
    g.write(reinterpret_cast<const char*>(bscandb.data()), bscandb.size() * sizeof(float));
    // and the first B-scan as an .ocv Mat dump (CV_32F, D x H), the format savematasbin uses
    ocv_write(out + "_bscan001.ocv", OD, OH, 5, bscan.data());
  }
  {
    // Matlab text, as savematasdata writes it (main:333-339: name "=" operator<<(Mat) ";"): rows separated by ";\n ",
    // columns by ", ", and every value with the 16 significant digits cv's default formatter gives a CV_64F Mat
    // (bscan is CV_64F in the reference, main:1220) -- enough to read the f32 results back exactly
    std::ofstream m(out + ".m");
    m << "bscan001=[";
    char num[40];
    for (int d = 0; d < OD; d++) {
      for (int r = 0; r < OH; r++) {
        std::snprintf(num, sizeof num, "%.16g", (double)bscan[(size_t)d * OH + r]);
        m << num;
        if (r + 1 < OH) m << ", ";
      }
      if (d + 1 < OD) m << ";\n ";
    }
    m << "];\n";
  }
  {
    // the display chain of main:1242-1255 + 1284 for the first B-scan, as portable grey/pix maps
    const size_t px = (size_t)OD * OH;
    std::vector<unsigned char> gray(px), bgr(3 * px);
    rc = fdoct_display(h, bscandb.data(), FDOCT_MEM_HOST, 1, OD, OH, bscanthreshold, 0, gray.data(),
                       bgr.data(), FDOCT_MEM_HOST);
    if (rc) {
      std::fprintf(stderr, "fdoct_display: %d %s\n", rc, fdoct_last_error(h));
      return 1;
    }
    std::ofstream pg(out + "_bscan001.pgm", std::ios::binary);
    pg << "P5\n" << OH << " " << OD << "\n255\n";
    pg.write(reinterpret_cast<const char*>(gray.data()), px);
    std::ofstream pp(out + "_bscanc001.ppm", std::ios::binary);
    pp << "P6\n" << OH << " " << OD << "\n255\n";
    for (size_t i = 0; i < px; i++) {  // cv::Mat colour order is B,G,R; PPM wants R,G,B
      const char rgb[3] = {(char)bgr[3 * i + 2], (char)bgr[3 * i + 1], (char)bgr[3 * i]};
      pp.write(rgb, 3);
    }
  }
  if (roi[0] >= 0) {
    // ROIreport: printAvgROI on each displayed B-scan (main:1289-1290), over the dB image after the DC mask
    std::vector<double> mean(G);
    rc = fdoct_roi_mean(h, bscandb.data(), FDOCT_MEM_HOST, FDOCT_LAYOUT_TRANSPOSED_DxH, G, OD, OH,
                        roi[0], roi[1], roi[2], mean.data(), FDOCT_MEM_HOST);
    if (rc) {
      std::fprintf(stderr, "fdoct_roi_mean: %d %s\n", rc, fdoct_last_error(h));
      return 1;
    }
    for (int g = 0; g < G; g++) std::printf("Mean of ROI at %d = %f dB\n", roi[0], mean[g]);
  }
  if (max_intensity) {
    // minMaxLoc(opmvector, &minVal, &maxVal) of the status line, main:1105-1108, per frame
    std::vector<double> mx(nframes);
    rc = fdoct_frame_minmax(h, live, dt, FDOCT_MEM_HOST, nframes, 0, nullptr, mx.data(), FDOCT_MEM_HOST);
    if (rc) {
      std::fprintf(stderr, "fdoct_frame_minmax: %d %s\n", rc, fdoct_last_error(h));
      return 1;
    }
    for (int f = 0; f < nframes; f++) std::printf("Max intensity = %d\n", int(std::floor(mx[f])));
  }
  for (fdoct_handle x : hs) fdoct_destroy(x);
  return 0;
}
