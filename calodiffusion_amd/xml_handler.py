"""``XMLHandler`` of the reference (calodiffusion/utils/XMLHandler.py): the CaloChallenge binning file of an irregular cylindrical
calorimeter, read with ``xml.etree``.

The format: one element per particle, ``<... name="photon">``, holding one element per calorimeter layer with the attributes
``id``, ``r_edges`` (comma-separated radial edges; a single value marks a layer without voxels) and ``n_bin_alpha``.  A layer's
voxels are ordered alpha-major, ``n_bin_alpha`` rows of ``len(r_edges) - 1`` radial bins, and the layers follow each other in the
flat shower: ``bin_edges`` holds their offsets.

This is what ``geom1.GeomConverter(bins=...)`` reads: ``r_edges``, ``alphaListPerLayer``, ``GetBinEdges()`` and
``GetRelevantLayers()``; ``r_bins``, ``a_bins``, ``bin_edges`` and ``GetTotalNumberOfBins()`` are kept for callers of the reference
class.

``eta_all_layers`` / ``phi_all_layers`` / ``GetEtaPhiAllLayers()`` are the voxel positions the reference derives in
``SetEtaAndPhiFromPolar`` (:72-108), which ``hlf.HighLevelFeatures`` weighs the energies with: per layer a float64 array in the flat
shower's voxel order, ``eta = r_mid * cos(alpha_centre)`` and ``phi = r_mid * sin(alpha_centre)``; a layer without voxels has an empty
array.  The reference's quirk is kept: ``GetRelevantLayers()`` holds layer INDICES and ``GetLayersWithBinningInAlpha()`` the XML
``id`` attributes, which differ where ids skip (Dataset 1's 0, 1, 2, 3, 12)."""
from __future__ import annotations

import math
import xml.etree.ElementTree as ET

import numpy as np


class XMLHandler:
    def __init__(self, particle_name, filename="binning.xml"):
        root = ET.parse(filename).getroot()
        self.r_bins, self.a_bins, self.r_edges, self.r_midvalue = [], [], [], []
        self.layerWithBinningInAlpha = []
        found = [particle for particle in root if particle.attrib.get("name") == particle_name]
        if not found:
            names = [particle.attrib.get("name") for particle in root]
            raise ValueError(f"Particle {particle_name} not found in {filename}, which has {names}")
        for particle in found:
            for layer in particle:
                self._read_layer(layer)
        self.minAlpha = -math.pi
        self.totalBins = 0
        self.bin_number, self.relevantlayers, self.alphaListPerLayer, self.nBinAlphaPerlayer = [], [], [], []
        for layer, (nr, na) in enumerate(zip(self.r_bins, self.a_bins)):
            self.totalBins += nr * na
            self.bin_number.append(nr * na)
            if nr > 0:
                centres = self._midpoints(np.linspace(self.minAlpha, math.pi, na + 1))
                self.relevantlayers.append(layer)
                self.alphaListPerLayer.append([centres for _ in range(nr)])
                self.nBinAlphaPerlayer.append([na] * nr)
            else:
                self.alphaListPerLayer.append([0])
                self.nBinAlphaPerlayer.append([0])
        self.bin_edges = [0]
        for n in self.bin_number:
            self.bin_edges.append(n + self.bin_edges[-1])
        self.eta_all_layers, self.phi_all_layers = [], []
        for layer, (nr, na) in enumerate(zip(self.r_bins, self.a_bins)):
            # alpha-major, r fastest (fill_r_a_lists, :72-83); a layer without voxels has no alpha bins either
            r_list = np.array(self.r_midvalue[layer] * (na if nr > 0 else 0), dtype=np.float64)
            a_list = [a for a in (self.alphaListPerLayer[layer][0] if nr > 0 else []) for _ in range(nr)]
            self.eta_all_layers.append(r_list * np.cos(np.array(a_list, dtype=np.float64)))
            self.phi_all_layers.append(r_list * np.sin(np.array(a_list, dtype=np.float64)))

    @staticmethod
    def _midpoints(arr):
        return [arr[i] + float(arr[i + 1] - arr[i]) / 2 for i in range(len(arr) - 1)]

    def _read_layer(self, elem):
        r_list = [float(s) for s in elem.attrib.get("r_edges").split(",")]
        self.r_edges.append(r_list)
        self.r_bins.append(len(r_list) - 1)
        n_alpha = int(elem.attrib.get("n_bin_alpha"))
        self.a_bins.append(n_alpha)
        self.r_midvalue.append(self._midpoints(r_list))
        if n_alpha > 1:
            self.layerWithBinningInAlpha.append(int(elem.attrib.get("id")))

    def GetTotalNumberOfBins(self):
        return self.totalBins

    def GetBinEdges(self):
        return self.bin_edges

    def GetEtaPhiAllLayers(self):
        return self.eta_all_layers, self.phi_all_layers

    def GetRelevantLayers(self):
        return self.relevantlayers

    def GetLayersWithBinningInAlpha(self):
        return self.layerWithBinningInAlpha
