// vtkm/cont/Algorithm.h: the VTK-m name the reference's worklet headers include, over tests/cpp/vtkm_min/vtkm_min.h.
#pragma once
#include <vtkm_min.h>
