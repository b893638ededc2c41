// TEST INFRASTRUCTURE.  Host half of the shape query API conformance check
// (see shapes_conformance.inl): plain host C++, as a simulator's Manager is.
#define SHAPESCONF_NAME shapesconf_host
#include "shapes_conformance.inl"
