// Glue for tests/golden/make_init_first_golden.py: runs the REFERENCE'S OWN CoarseInitializer::setFirst (with makeNN) and its own makePixelStatus (PixelSelector.h) on a
// frame given as an image (the sources compiled into oracle/_ref/libref.so by oracle/Makefile.ref).  Nothing of the reference is restated here: the glue builds the
// FrameHessian, sets the global sparsityFactor, calls the member / the function, and reads members back.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#define private public
#define protected public
#include "util/NumType.h"
#include "util/settings.h"
#include "util/globalCalib.h"
#include "util/FrameShell.h"
#include "FullSystem/HessianBlocks.h"
#include "FullSystem/CoarseInitializer.h"
#include "FullSystem/PixelSelector.h"
#include "FullSystem/PixelSelector2.h"
#undef private
#undef protected

using namespace dso;

struct Glue {
	CoarseInitializer* ci;
	CalibHessian* calib;
	FrameHessian* fh;
	int w, h;
};

extern "C" {

void* ifg_create(int w, int h, const float* K4, const float* img, int* levels)
{
	Eigen::Matrix3f K = Eigen::Matrix3f::Identity();
	K(0, 0) = K4[0]; K(1, 1) = K4[1]; K(0, 2) = K4[2]; K(1, 2) = K4[3];
	setGlobalCalib(w, h, K);
	multiThreading = false;
	Glue* g = new Glue();
	g->w = w; g->h = h;
	g->calib = new CalibHessian();
	VecC kv; kv << K4[0], K4[1], K4[2], K4[3];
	g->calib->setValueScaled(kv);
	g->ci = new CoarseInitializer(w, h);
	g->ci->printDebug = false;
	FrameHessian* fh = new FrameHessian();
	FrameShell* shell = new FrameShell();
	shell->camToWorld = SE3();
	shell->aff_g2l = AffLight(0, 0);
	shell->marginalizedAt = shell->id = 0;
	shell->timestamp = 0;
	shell->incoming_id = 0;
	fh->shell = shell;
	fh->ab_exposure = 0;
	std::vector<float> copy(img, img + (size_t)w * h);
	fh->makeImages(copy.data(), g->calib);
	// rows 0 and h-1 of the three absSquaredGrad planes the level-0 selector reads, which makeImages leaves unwritten, are zeroed (as pixel_select_glue.cpp does): the
	// selector reads the last row of level 2 for the pixels of row h-4, and what a recycled heap block holds there would change the selection from run to run
	for (int l = 0; l < 3; l++)
	{
		memset(fh->absSquaredGrad[l], 0, sizeof(float) * wG[l]);
		memset(fh->absSquaredGrad[l] + (size_t)wG[l] * (hG[l] - 1), 0, sizeof(float) * wG[l]);
	}
	g->fh = fh;
	*levels = pyrLevelsUsed;
	return g;
}
void ifg_destroy(void* p)
{
	Glue* g = (Glue*)p;
	g->ci->firstFrame = 0; g->ci->newFrame = 0;
	delete g->ci;
	g->fh->efFrame = 0;
	FrameShell* s = g->fh->shell;
	delete g->fh; delete s;
	delete g->calib;
	delete g;
}
// randomPattern of a PixelSelector made the way setFirst makes its own (:810)
void ifg_pattern(void* p, unsigned char* out)
{
	Glue* g = (Glue*)p;
	PixelSelector sel(g->w, g->h);
	memcpy(out, sel.randomPattern, (size_t)g->w * g->h);
}
// CoarseInitializer::setFirst with the global sparsityFactor set before and read after; returns the wall time of the call in seconds
double ifg_set_first(void* p, int sparsity_in, int* sparsity_out, int* n_points)
{
	Glue* g = (Glue*)p;
	sparsityFactor = sparsity_in;
	const auto t0 = std::chrono::steady_clock::now();
	g->ci->setFirst(g->calib, g->fh);
	const auto t1 = std::chrono::steady_clock::now();
	*sparsity_out = sparsityFactor;
	for (int l = 0; l < pyrLevelsUsed; l++) n_points[l] = g->ci->numPoints[l];
	return std::chrono::duration<double>(t1 - t0).count();
}
void ifg_get_level(void* p, int lvl, float* u, float* v, float* my_type, float* outlierTH, int* neighbours10, int* parent)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	for (int i = 0; i < ci->numPoints[lvl]; i++)
	{
		const Pnt& q = ci->points[lvl][i];
		u[i] = q.u; v[i] = q.v; my_type[i] = q.my_type; outlierTH[i] = q.outlierTH;
		for (int k = 0; k < 10; k++) neighbours10[10 * i + k] = q.neighbours[k];
		parent[i] = q.parent;
	}
}
// makePixelStatus on dIp[lvl] of the frame; returns numGood, map_out: w_lvl * h_lvl bytes
int ifg_make_pixel_status(void* p, int lvl, float desiredDensity, int recsLeft, float THFac, int sparsity_in, int* sparsity_out, unsigned char* map_out)
{
	Glue* g = (Glue*)p;
	const int wl = g->w >> lvl, hl = g->h >> lvl;
	bool* map = new bool[(size_t)wl * hl];
	sparsityFactor = sparsity_in;
	const int n = makePixelStatus(g->fh->dIp[lvl], map, wl, hl, desiredDensity, recsLeft, THFac);
	*sparsity_out = sparsityFactor;
	for (int i = 0; i < wl * hl; i++) map_out[i] = map[i] ? 1 : 0;
	delete[] map;
	return n;
}
// dIp[lvl] of the frame: (I, dx, dy) per pixel
void ifg_get_dI(void* p, int lvl, float* out3)
{
	Glue* g = (Glue*)p;
	const int wl = g->w >> lvl, hl = g->h >> lvl;
	for (int i = 0; i < wl * hl; i++) for (int k = 0; k < 3; k++) out3[3 * i + k] = g->fh->dIp[lvl][i][k];
}

}  // extern "C"
