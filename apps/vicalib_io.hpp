// The command-line tool's file readers and writers: 8- and 16-bit PGM images, detections, IMU logs, camera model and rig files, pose files,
// depth correction files.  A piece of vicalib.cpp's translation unit: that file includes it behind the system headers, nothing else does.
#pragma once
// ------------------------------------------------------------------------------------------- inputs
static std::vector<std::string> Split(const std::string& s, char sep) {
  std::vector<std::string> out; std::stringstream ss(s); std::string item;
  while (std::getline(ss, item, sep)) if (!item.empty()) out.push_back(item);
  return out;
}
static std::string StripScheme(const std::string& uri) {
  const size_t p = uri.find("//");
  return p == std::string::npos ? uri : uri.substr(p + 2);
}
static bool ParseNumbers(const std::string& line, std::vector<double>* v) {
  v->clear();
  const char* p = line.c_str();
  while (*p) {
    while (*p == ' ' || *p == '\t' || *p == ',' || *p == ';' || *p == '\r') ++p;
    if (!*p) break;
    char* end = nullptr;
    const double d = std::strtod(p, &end);
    if (end == p) return false;
    v->push_back(d); p = end;
  }
  return !v->empty();
}

struct Detection { long frame; int dot; double u, v, X, Y, Z; };
struct Channel { std::vector<Detection> det; std::map<long, double> frame_time; };
// frame id -> position in ids
static std::map<long, int> FrameIndex(const std::vector<long>& ids) {
  std::map<long, int> index;
  for (size_t k = 0; k < ids.size(); ++k) index[ids[k]] = (int)k;
  return index;
}
// A channel's detections in the frames of `index` (frame id -> frame number), dots outside the grid of grid_n dots dropped (vicalib-task.cc:353-354):
// one list per frame number, ascending, each in the order of the file.  The pointers stay valid as long as ch.det does not move.
static std::map<int, std::vector<const Detection*>> DetectionsByFrame(const Channel& ch, const std::map<long, int>& index, int grid_n) {
  std::map<int, std::vector<const Detection*>> per_frame;
  for (const Detection& d : ch.det) {
    auto it = index.find(d.frame);
    if (it != index.end() && d.dot < grid_n) per_frame[it->second].push_back(&d);
  }
  return per_frame;
}
// ... flattened behind pw (X Y Z per corner) and pc (u v per corner)
static void AppendCorners(const std::vector<const Detection*>& dets, std::vector<double>* pw, std::vector<double>* pc) {
  for (const Detection* d : dets) { pw->insert(pw->end(), {d->X, d->Y, d->Z}); pc->insert(pc->end(), {d->u, d->v}); }
}
// this frame id's time: the first channel that has one, else id / frame_rate
static double FrameTime(const std::vector<Channel>& channels, long id) {
  for (const Channel& ch : channels) { auto it = ch.frame_time.find(id); if (it != ch.frame_time.end()) return it->second; }
  return (double)id / FlagDouble("frame_rate");
}

// ---- image channels (vicalib-task.cc:263-330 with files for sensors) ----------------------------------------------------------------
static bool ReadPgm(const std::string& path, int* w, int* h, std::vector<unsigned char>* px, std::string* err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { *err = "cannot open image " + path; return false; }
  std::string magic; f >> magic;
  if (magic != "P5") { *err = path + ": not a binary PGM (P5)"; return false; }
  auto next_int = [&](long* v) {
    while (true) { f >> std::ws; if (f.peek() == '#') { std::string c; std::getline(f, c); } else break; }
    return (bool)(f >> *v);
  };
  long W = 0, H = 0, M = 0;
  if (!next_int(&W) || !next_int(&H) || !next_int(&M) || W < 1 || H < 1 || M != 255) { *err = path + ": expected an 8-bit PGM header"; return false; }
  f.get();                                          // the single whitespace byte behind the header
  px->resize((size_t)W * H);
  f.read((char*)px->data(), (std::streamsize)px->size());
  if ((size_t)f.gcount() != px->size()) { *err = path + ": truncated image data"; return false; }
  *w = (int)W; *h = (int)H;
  return true;
}
static bool GlobSorted(const std::string& pattern_glob, std::vector<std::string>* files) {
  glob_t g; std::memset(&g, 0, sizeof(g));
  const bool ok = glob(pattern_glob.c_str(), 0, nullptr, &g) == 0 && g.gl_pathc > 0;
  if (ok) files->assign(g.gl_pathv, g.gl_pathv + g.gl_pathc);
  globfree(&g);
  std::sort(files->begin(), files->end());
  return ok;
}
struct TargetSpec { std::vector<int> pattern; int rows = 0, cols = 0; double spacing = 0.0; };
// one camera channel from a glob of images: frame k = k-th file (sorted); detections carry the target dot's index and position
static bool ReadImages(const std::string& pattern_glob, const TargetSpec& tg, int device, Channel* ch, int* width, int* height, std::string* err) {
  std::vector<std::string> files;
  if (!GlobSorted(pattern_glob, &files)) { *err = "no images match " + pattern_glob; return false; }
  vc_detector* det = nullptr;
  std::vector<unsigned char> px;
  const int kMax = 4096;
  std::vector<double> cen(2 * kMax), con(9 * kMax);
  std::vector<int> box(4 * kMax), idx(kMax);
  long placed = 0, skipped = 0;
  for (size_t k = 0; k < files.size(); ++k) {
    int w = 0, h = 0;
    if (!ReadPgm(files[k], &w, &h, &px, err)) { if (det) vc_detector_destroy(det); return false; }
    if (!det) {
      const int rc = vc_detector_create(device, w, h, &det);
      if (rc != VC_OK) { *err = rc == VC_ERR_NO_DEVICE ? "no usable HIP device for the dot detector" : "vc_detector_create failed"; return false; }
      *width = w; *height = h;
    } else if (w != *width || h != *height) { *err = files[k] + ": image size differs from the first image of the channel"; vc_detector_destroy(det); return false; }
    int n = 0, m = 0;
    if (vc_detector_find_conics(det, px.data(), w, cen.data(), con.data(), box.data(), kMax, &n) != VC_OK ||
        vc_target_find(cen.data(), con.data(), n, tg.pattern.data(), tg.rows, tg.cols, idx.data(), &m) != VC_OK) { *err = files[k] + ": detection failed"; vc_detector_destroy(det); return false; }
    if (m == 0) { ++skipped; continue; }                 // "Tracking bad" (vicalib-task.cc:278-281): the frame contributes nothing
    for (int i = 0; i < n; ++i) {
      if (idx[i] < 0) continue;
      const int r = idx[i] / tg.cols, c = idx[i] % tg.cols;
      ch->det.push_back(Detection{(long)k, idx[i], cen[2 * i], cen[2 * i + 1], c * tg.spacing, r * tg.spacing, 0.0});
      ++placed;
    }
  }
  if (det) vc_detector_destroy(det);
  std::fprintf(stderr, "I %s: %zu images, %ld dots associated with the target, %ld images without an unambiguous placement\n", pattern_glob.c_str(), files.size(), placed, skipped);
  return true;
}
static bool ReadDetections(const std::string& path, Channel* ch, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open detections file " + path; return false; }
  std::string line; std::vector<double> v; long ln = 0;
  while (std::getline(f, line)) {
    ++ln;
    if (line.empty() || line[0] == '#' || line[0] == '%') continue;
    if (!ParseNumbers(line, &v)) continue;                    // header / log text between the detection lines
    if (v.size() < 7) { *err = path + ":" + std::to_string(ln) + ": expected frame,dot_id,u,v,X,Y,Z[,time]"; return false; }
    if (v[1] < 0) continue;                                   // unmatched conic (vicalib-task.cc:309-311)
    ch->det.push_back(Detection{(long)v[0], (int)v[1], v[2], v[3], v[4], v[5], v[6]});
    if (v.size() >= 8) ch->frame_time[(long)v[0]] = v[7];
  }
  return true;
}

struct ImuData { std::vector<double> gyro, accel, time; };
static bool ReadColumns(const std::string& path, int min_cols, std::vector<std::vector<double>>* rows, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open " + path; return false; }
  std::string line; std::vector<double> v;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#' || line[0] == '%') continue;
    if (!ParseNumbers(line, &v)) continue;
    if ((int)v.size() < min_cols) { *err = path + ": expected at least " + std::to_string(min_cols) + " columns"; return false; }
    rows->push_back(v);
  }
  return true;
}
static bool ReadImu(const std::string& dir, bool system_time, ImuData* imu, std::string* err) {
  std::vector<std::vector<double>> a, g, t;
  if (!ReadColumns(dir + "/accel.txt", 3, &a, err) || !ReadColumns(dir + "/gyro.txt", 3, &g, err) || !ReadColumns(dir + "/timestamp.txt", 1, &t, err)) return false;
  const size_t n = std::min(a.size(), std::min(g.size(), t.size()));
  double last = -1e300;
  for (size_t i = 0; i < n; ++i) {
    const double ts = (!system_time && t[i].size() > 1) ? t[i][1] : t[i][0];
    if (ts <= last) continue;                                 // the calibrator insists on strictly increasing time (vicalibrator.h:373-378)
    last = ts;
    imu->time.push_back(ts);
    for (int k = 0; k < 3; ++k) { imu->gyro.push_back(g[i][k]); imu->accel.push_back(a[i][k]); }
  }
  return true;
}

static int ModelId(const std::string& type) {     // -models strings (vicalib-engine.cc:203-253) and XML type strings (:210-260)
  if (type == "fov" || type == "calibu_fu_fv_u0_v0_w") return VC_MODEL_FOV;
  if (type == "poly2" || type == "calibu_fu_fv_u0_v0_k1_k2") return VC_MODEL_POLY2;
  if (type == "poly3" || type == "poly" || type == "calibu_fu_fv_u0_v0_k1_k2_k3") return VC_MODEL_POLY3;
  if (type == "kb4" || type == "calibu_fu_fv_u0_v0_kb4") return VC_MODEL_KB4;
  if (type == "linear" || type == "calibu_fu_fv_u0_v0") return VC_MODEL_LINEAR;
  if (type == "rational6" || type == "rational" || type == "calibu_fu_fv_u0_v0_rational6") return VC_MODEL_RATIONAL6;      // vicalib-engine.cc:233-240
  return -1;
}
static const char* ModelName(int id) { static const char* n[] = {"fov", "poly2", "poly3", "kb4", "linear", "rational6"}; return (id >= 0 && id < 6) ? n[id] : "?"; }

static std::string Between(const std::string& s, const std::string& a, const std::string& b, size_t from = 0) {
  const size_t p = s.find(a, from); if (p == std::string::npos) return "";
  const size_t q = s.find(b, p + a.size()); if (q == std::string::npos) return "";
  return s.substr(p + a.size(), q - p - a.size());
}
// first <camera_model> of a calibu rig XML (the reference takes rig->cameras_[0], pose ignored: vicalib-engine.cc:190-197)
static bool ReadModelFile(const std::string& path, vic::CameraAndPose* cam, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open model file " + path; return false; }
  std::stringstream ss; ss << f.rdbuf();
  const std::string s = ss.str();
  const std::string head = Between(s, "<camera_model", ">");
  cam->model = ModelId(Between(head, "type=\"", "\""));
  if (cam->model < 0) { *err = path + ": unsupported camera model type '" + Between(head, "type=\"", "\"") + "'"; return false; }
  std::vector<double> v;
  if (ParseNumbers(Between(s, "<width>", "</width>"), &v)) cam->width = (int)v[0];
  if (ParseNumbers(Between(s, "<height>", "</height>"), &v)) cam->height = (int)v[0];
  std::string p = Between(s, "<params>", "</params>");
  std::replace(p.begin(), p.end(), '[', ' '); std::replace(p.begin(), p.end(), ']', ' ');
  if (!ParseNumbers(p, &cam->params)) { *err = path + ": no <params>"; return false; }
  return true;
}
static bool WritePgm(const std::string& path, int w, int h, const unsigned char* px, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) { *err = "cannot write " + path; return false; }
  std::fprintf(f, "P5\n%d %d\n255\n", w, h);
  std::fwrite(px, 1, (size_t)w * h, f);
  std::fclose(f);
  return true;
}
static std::string BaseName(std::string name) {
  const size_t slash = name.find_last_of('/');
  if (slash != std::string::npos) name = name.substr(slash + 1);
  const size_t dot = name.find_last_of('.');
  if (dot != std::string::npos && dot > 0) name = name.substr(0, dot);
  return name;
}
// every <camera> of a calibu rig XML with its pose: the inverse of vc_write_camera_models.  T_wc = [M | t] with M = R_ck^T RDF^T and
// t = -R_ck^T t_ck, RDF the matrix of the <right>, <down> and <forward> rows (the identity when they are missing).
static bool ReadRigFile(const std::string& path, std::vector<vic::CameraAndPose>* cams, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open rig file " + path; return false; }
  std::stringstream ss; ss << f.rdbuf();
  const std::string s = ss.str();
  cams->clear();
  auto numbers = [](std::string t, std::vector<double>* v) {
    for (char& ch : t) if (ch == '[' || ch == ']') ch = ' ';
    return ParseNumbers(t, v);
  };
  for (size_t from = 0;;) {
    const size_t p = s.find("<camera>", from);
    if (p == std::string::npos) break;
    const size_t q = s.find("</camera>", p);
    if (q == std::string::npos) { *err = path + ": <camera> without </camera>"; return false; }
    const std::string c = s.substr(p, q - p);
    from = q + 9;
    const std::string where = path + ": camera " + std::to_string(cams->size());
    vic::CameraAndPose cam;
    const std::string head = Between(c, "<camera_model", ">");
    cam.model = ModelId(Between(head, "type=\"", "\""));
    if (cam.model < 0) { *err = where + ": unsupported camera model type '" + Between(head, "type=\"", "\"") + "'"; return false; }
    std::vector<double> v;
    if (!numbers(Between(c, "<width>", "</width>"), &v) || v.size() != 1 || !(v[0] >= 2 && v[0] <= 8192)) { *err = where + ": no usable <width>"; return false; }
    cam.width = (int)v[0];
    if (!numbers(Between(c, "<height>", "</height>"), &v) || v.size() != 1 || !(v[0] >= 2 && v[0] <= 8192)) { *err = where + ": no usable <height>"; return false; }
    cam.height = (int)v[0];
    static const int kParams[6] = {5, 6, 7, 8, 4, 10};
    if (!numbers(Between(c, "<params>", "</params>"), &cam.params) || (int)cam.params.size() != kParams[cam.model]) {
      *err = where + ": <params> does not hold the " + std::to_string(kParams[cam.model]) + " parameters of " + ModelName(cam.model); return false;
    }
    double rdf[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const char* rows[3] = {"right", "down", "forward"};
    for (int r = 0; r < 3; ++r) {
      const std::string t = Between(c, std::string("<") + rows[r] + ">", std::string("</") + rows[r] + ">");
      if (t.empty()) continue;
      if (!numbers(t, &v) || v.size() != 3) { *err = where + ": <" + rows[r] + "> does not hold 3 numbers"; return false; }
      for (int k = 0; k < 3; ++k) rdf[3 * r + k] = v[k];
    }
    if (!numbers(Between(c, "<T_wc>", "</T_wc>"), &v) || v.size() != 12) { *err = where + ": <T_wc> does not hold 3 x 4 numbers"; return false; }
    // R_ck^T = M RDF; R_ck = its transpose; t_ck = -R_ck t
    double Rt[9], R[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rt[3 * i + j] = v[4 * i] * rdf[j] + v[4 * i + 1] * rdf[3 + j] + v[4 * i + 2] * rdf[6 + j];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[3 * i + j] = Rt[3 * j + i];
    double ortho = 0.0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
      ortho = std::max(ortho, std::fabs(R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0)));
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(ortho <= 1e-6) || !(det > 0.0)) { *err = where + ": <T_wc> and the axis rows do not give a rotation"; return false; }
    double* T = cam.T_ck.data();
    // Shepperd: the unit quaternion [x y z w] of R_ck
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) { const double k = 2.0 * std::sqrt(tr + 1.0); T[3] = 0.25 * k; T[0] = (R[7] - R[5]) / k; T[1] = (R[2] - R[6]) / k; T[2] = (R[3] - R[1]) / k; }
    else if (R[0] > R[4] && R[0] > R[8]) { const double k = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]); T[3] = (R[7] - R[5]) / k; T[0] = 0.25 * k; T[1] = (R[1] + R[3]) / k; T[2] = (R[2] + R[6]) / k; }
    else if (R[4] > R[8]) { const double k = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]); T[3] = (R[2] - R[6]) / k; T[0] = (R[1] + R[3]) / k; T[1] = 0.25 * k; T[2] = (R[5] + R[7]) / k; }
    else { const double k = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]); T[3] = (R[3] - R[1]) / k; T[0] = (R[2] + R[6]) / k; T[1] = (R[5] + R[7]) / k; T[2] = 0.25 * k; }
    const double qn = std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2] + T[3] * T[3]);
    for (int k = 0; k < 4; ++k) T[k] /= qn;
    for (int i = 0; i < 3; ++i) T[4 + i] = -(R[3 * i] * v[3] + R[3 * i + 1] * v[7] + R[3 * i + 2] * v[11]);
    cams->push_back(cam);
  }
  if (cams->empty()) { *err = path + ": no <camera>"; return false; }
  return true;
}
// 16-bit binary PGM, maxval 65535, most significant byte first (the Netpbm rule)
static bool ReadPgm16(const std::string& path, int* w, int* h, std::vector<unsigned short>* px, std::string* err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { *err = "cannot open image " + path; return false; }
  std::string magic; f >> magic;
  if (magic != "P5") { *err = path + ": not a binary PGM (P5)"; return false; }
  auto next_int = [&](long* v) {
    while (true) { f >> std::ws; if (f.peek() == '#') { std::string c; std::getline(f, c); } else break; }
    return (bool)(f >> *v);
  };
  long W = 0, H = 0, M = 0;
  if (!next_int(&W) || !next_int(&H) || !next_int(&M) || W < 1 || H < 1 || M != 65535) { *err = path + ": expected a 16-bit PGM header (maxval 65535)"; return false; }
  if (W > 8192 || H > 8192) { *err = path + ": " + std::to_string(W) + " x " + std::to_string(H) + " pixels, more than the 8192 x 8192 a camera can have"; return false; }
  f.get();                                          // the single whitespace byte behind the header
  std::vector<unsigned char> raw((size_t)W * H * 2);
  f.read((char*)raw.data(), (std::streamsize)raw.size());
  if ((size_t)f.gcount() != raw.size()) { *err = path + ": truncated image data"; return false; }
  px->resize((size_t)W * H);
  for (size_t k = 0; k < px->size(); ++k) (*px)[k] = (unsigned short)((raw[2 * k] << 8) | raw[2 * k + 1]);
  *w = (int)W; *h = (int)H;
  return true;
}
static bool WritePgm16(const std::string& path, int w, int h, const unsigned short* px, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) { *err = "cannot write " + path; return false; }
  std::fprintf(f, "P5\n%d %d\n65535\n", w, h);
  std::vector<unsigned char> raw((size_t)w * h * 2);
  for (size_t k = 0; k < (size_t)w * h; ++k) { raw[2 * k] = (unsigned char)(px[k] >> 8); raw[2 * k + 1] = (unsigned char)(px[k] & 255); }
  const bool written = std::fwrite(raw.data(), 1, raw.size(), f) == raw.size();
  if (std::fclose(f) != 0 || !written) { *err = "cannot write " + path + " in full"; return false; }
  return true;
}
// a pose file in the format -save_poses writes: lines of 12 numbers, the top three rows of T_wk, '%' starts a comment -> [q (x y z w), t]
static bool ReadPoseFile(const std::string& path, std::vector<std::array<double, 7>>* poses, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open pose file " + path; return false; }
  std::string line;
  while (std::getline(f, line)) {
    if (line.find_first_not_of(" \t\r") == std::string::npos || line[line.find_first_not_of(" \t\r")] == '%') continue;
    double m[12];
    std::istringstream is(line);
    for (int k = 0; k < 12; ++k) if (!(is >> m[k])) { *err = path + ": expected 12 numbers in a line"; return false; }
    const double R[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
    double q[4];                                         // the largest of the four components first (Shepperd), then unit length
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) { const double s = std::sqrt(tr + 1.0) * 2.0; q[3] = 0.25 * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; }
    else if (R[0] > R[4] && R[0] > R[8]) { const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0; q[3] = (R[7] - R[5]) / s; q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; }
    else if (R[4] > R[8]) { const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0; q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s; }
    else { const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0; q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s; }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(n > 0.5 && n < 2.0)) { *err = path + ": a line holds no rotation"; return false; }
    poses->push_back({{q[0] / n, q[1] / n, q[2] / n, q[3] / n, m[3], m[7], m[11]}});
  }
  return true;
}
static bool ReadDepthFiles(const std::vector<std::string>& files, int w, int h, const std::string& who, std::vector<unsigned short>* depth, std::string* err) {
  for (size_t k = 0; k < files.size(); ++k) {
    int fw = 0, fh = 0;
    std::vector<unsigned short> px;
    if (!ReadPgm16(files[k], &fw, &fh, &px, err)) return false;
    if (k == 0 && w == 0) { w = fw; h = fh; }
    if (fw != w || fh != h) { *err = files[k] + ": " + std::to_string(fw) + " x " + std::to_string(fh) + " pixels, " + who + " has " + std::to_string(w) + " x " + std::to_string(h); return false; }
    depth->insert(depth->end(), px.begin(), px.end());
  }
  return true;
}
static bool MakeDir(const std::string& dir, std::string* err) {
  struct stat st;
  if (mkdir(dir.c_str(), 0777) != 0 && !(stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "cannot create the directory " + dir; return false; }      // (one level)
  return true;
}
struct DepthCorrectionFile { int w = 0, h = 0, bx = 0, by = 0, degree = 0; double v_ref = 0, unit = 0, c[3] = {0, 0, 0}; std::vector<double> a, b; };
static bool ReadDepthCorrection(const std::string& path, DepthCorrectionFile* f, std::string* err) {
  std::ifstream in(path);
  if (!in) { *err = "cannot open correction file " + path; return false; }
  std::string line;
  bool ok = true;
  auto header = [&](const char* fmt, auto... ptr) { ok = ok && std::getline(in, line) && std::sscanf(line.c_str(), fmt, ptr...) == (int)sizeof...(ptr); };
  header("size,%d,%d", &f->w, &f->h); header("bins,%d,%d", &f->bx, &f->by); header("v_ref,%lf", &f->v_ref); header("unit,%lf", &f->unit); header("degree,%d", &f->degree);
  header("c,%lf,%lf,%lf", &f->c[0], &f->c[1], &f->c[2]);
  ok = ok && std::getline(in, line) && line.compare(0, 5, "cx,cy") == 0;
  if (!ok || f->w < 2 || f->h < 2 || f->w > 8192 || f->h > 8192 || f->bx < 1 || f->by < 1 || f->bx > 32 || f->by > 32 || f->degree < 0 || f->degree > 2 || !(f->v_ref > 0.0) ||
      !(f->unit > 0.0)) { *err = path + ": not a depth correction file"; return false; }
  f->a.assign((size_t)f->bx * f->by, 0.0); f->b = f->a;
  for (int k = 0; k < f->bx * f->by; ++k) {
    int cx, cy, st; double n;
    if (!std::getline(in, line) || std::sscanf(line.c_str(), "%d,%d,%lf,%d,%lf,%lf", &cx, &cy, &n, &st, &f->a[k], &f->b[k]) != 6 || cx != k % f->bx || cy != k / f->bx) {
      *err = path + ": expected the row of cell " + std::to_string(k); return false;
    }
  }
  return true;
}
